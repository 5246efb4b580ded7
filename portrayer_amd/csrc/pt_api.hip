// The C ABI declared in include/portrayer_hip.h: the context's life cycle, render calls and the passes beside the render, and the
// small kernels around the render kernel (finishing pass, untile, explicit-ray casts for the parity tests). The scene - upload (tree builds), update,
// deform - is in pt_scene.hip; the context both units share in pt_context.h.
// The render kernel itself is in pt_render_kernel.h, instantiated per traversal mode by pt_render_inst.hip.
#include <type_traits>

#include "pt_context.h"
#include "pt_aov_inst.h"
#include "pt_guides_inst.h"
#include "pt_chart.h"
#include "pt_rays_inst.h"
#include "pt_segments_inst.h"
#include "pt_ao_inst.h"
#include "pt_direct_inst.h"
#include "pt_radiance_inst.h"
#include "pt_gather_inst.h"
#include "pt_probe_inst.h"
#include "pt_film_inst.h"
#include "pt_lens_inst.h"
#include "pt_film_map_inst.h"
#include "pt_denoise.h"
#include "pt_render_inst.h"
#include "pt_shade.h"
#include "pt_pixel_list.h"

// ------------------------------------------------------------------------------------------------
// Kernels
// ------------------------------------------------------------------------------------------------
template <int MODE>
__global__ void __launch_bounds__(PT_BLOCK) pt_cast_kernel(PtSceneView sc, uint64_t n, const double* o, const double* d, int any,
                                                          double* out_t, int32_t* out_node, int32_t* out_sub, unsigned int* overflow) {
    extern __shared__ uint32_t pt_lds[];
    PtStack stk;
    stk.base = pt_lds + threadIdx.x;
    stk.cap = sc.stack_cap;
    stk.overflow = overflow;
    uint64_t i = (uint64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (i >= n) return;
    PtRay r;
    r.o = pt_v3(o[3 * i], o[3 * i + 1], o[3 * i + 2]);
    r.d = pt_v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
    PtHit hit;
    PtCounters cnt;
    pt_trace<MODE, false>(sc, r, any != 0, hit, stk, &cnt);
    out_t[i] = hit.node == PT_NO_HIT ? INFINITY : hit.t;
    out_node[i] = hit.node == PT_NO_HIT ? -1 : (int32_t)hit.node;
    out_sub[i] = hit.node == PT_NO_HIT ? -1 : (int32_t)hit.sub;
}

__global__ void pt_math_kernel(int op, uint64_t n, const double* a, const double* b, double* out) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double r;
    switch (op) {
    case 0: r = sqrt(a[i]); break;
    case 1: r = a[i] / b[i]; break;
    case 2: r = pt_pow(a[i], b[i]); break;  // the kernels' pow (pt_pow.h: glibc's, bit for bit)
    case 3: r = a[i] * b[i] + a[i]; break;  // must NOT be fused (-ffp-contract=off)
    case 4: r = atan2(a[i], b[i]); break;   // sphere.rs:57-58 (texture coordinates)
    case 5: r = acos(a[i]); break;          // sphere.rs:59
    case 6: r = pow(a[i], b[i]); break;     // the device library's pow, for comparison
    case 7:  // the k-d walk's short division (pt_walk_kd.h: pt_div_fast) where its exponent test admits the operands, NaN where it does not
        r = (pt_div_exp_ok(a[i]) && pt_div_exp_ok(b[i])) ? pt_div_fast(a[i], b[i], pt_rcp_refined(b[i])) : __builtin_nan("");
        break;
    default: r = 0.0; break;
    }
    out[i] = r;
}

__global__ void __launch_bounds__(256) pt_copy_kernel(const double2* __restrict__ src, double2* __restrict__ dst, size_t n) {
    // four independent 16-byte loads in flight per lane before the first store
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n; i += 4 * stride) {
        double2 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
        dst[i] = a; dst[i + stride] = b; dst[i + 2 * stride] = c; dst[i + 3 * stride] = d;
    }
    for (; i < n; i += stride) dst[i] = src[i];
}

// the plainest form: one 16-byte element per thread, as many blocks as it takes
__global__ void __launch_bounds__(256) pt_copy1_kernel(const double2* __restrict__ src, double2* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// Second pass of a render: chunk sums -> pixels, a block of PT_BLOCK threads per PT_BLOCK pixel slots. The chunk sums are pixel-major (the
// render kernel's chunk-first lanes write one pixel's sums side by side), so a thread per pixel would read 24 bytes every 24 x n_chunks
// bytes; instead the block first adds them up EIGHT THREADS PER PIXEL - thread j of a pixel holds chunk 8 b + j of the b-th block of eight,
// its seven neighbours' loads next to it, and the pixel's first thread adds the eight values in ascending order (the summation contract: a
// fixed left-to-right association) - leaves the sums in LDS, and then finishes ONE pixel per thread (the three pows with every lane busy).
// has_queue (launches whose list kernel left the masks of the pixels that need the render kernel, pt_pixel_list.h - found through a.eye_tab, 8 bytes per tile of 64
// pixel slots): a pixel whose bit is clear was never dealt, and nothing wrote its chunk sums. Inside the slice that is a pixel whose record is {no entry, nothing left
// out, unmarked}: its thread computes the sum from the background alone (pt_background_sum: the same adds in the same order), and the eight-threads-per-pixel loads are
// skipped for it. (Outside the slice pt_finish_pixel writes nothing, as ever.)
__global__ void __launch_bounds__(PT_BLOCK) pt_finish_kernel(PtRenderArgs a, uint32_t has_queue) {
    __shared__ double sums[3 * PT_BLOCK];
    const uint32_t base = blockIdx.x * PT_BLOCK, j = threadIdx.x & 7u;
#ifndef PT_NO_BACKGROUND_SKIP
    const unsigned long long* masks = nullptr;
    if (has_queue) masks = pt_pl_masks((uint32_t*)((char*)a.eye_tab + pt_pl_header_offset((uint32_t)a.scene.n_nodes) + 64u), a.n_slots);
    // slot p was dealt to the render kernel (p < n_slots; has_queue)
    auto dealt = [&](uint32_t p) { return ((masks[p >> 6] >> pt_pl_slot_to_tile_order(p & 63u)) & 1ull) != 0ull; };
#endif
    for (uint32_t pass = 0; pass < 8u; pass++) {
        const uint32_t local = pass * (PT_BLOCK / 8u) + (threadIdx.x >> 3), p = base + local;
        PtVec3 sum = pt_v3(0.0, 0.0, 0.0);
#ifndef PT_NO_BACKGROUND_SKIP
        const bool skip = has_queue && p < a.n_slots && !dealt(p);
#else
        const bool skip = false;
#endif
        for (uint32_t b = 0; b < a.n_chunks; b += 8u) {  // (wave-uniform trip count)
            const uint32_t k = b + j;
            PtVec3 v = pt_v3(0.0, 0.0, 0.0);
            if (p < a.n_slots && k < a.n_chunks && !skip) { const double* c = a.accum + 3 * ((size_t)p * a.n_chunks + k); v = pt_v3(c[0], c[1], c[2]); }
            const uint32_t n = a.n_chunks - b < 8u ? a.n_chunks - b : 8u;
            for (uint32_t i = 0; i < n; i++) {  // chunk b + i of this pixel, from thread i of its eight
                const int src = (int)((threadIdx.x & 63u & ~7u) + i);
                const PtVec3 w = pt_v3(__shfl(v.x, src), __shfl(v.y, src), __shfl(v.z, src));
                sum = (b == 0u && i == 0u) ? w : sum + w;
            }
        }
        if (j == 0u) { sums[3 * local] = sum.x; sums[3 * local + 1] = sum.y; sums[3 * local + 2] = sum.z; }
    }
    __syncthreads();
    const uint32_t p = base + threadIdx.x;
    if (p >= a.n_slots) return;
    PtVec3 sum = pt_v3(sums[3 * threadIdx.x], sums[3 * threadIdx.x + 1], sums[3 * threadIdx.x + 2]);
#ifndef PT_NO_BACKGROUND_SKIP
    if (has_queue && !dealt(p)) {
        uint32_t x, y;
        if (!pt_slot_to_pixel(a, p, &x, &y)) return;  // (pt_finish_pixel's own test: a slot outside the slice has no background to read)
        sum = pt_background_sum(a, x, y);
    }
#endif
    pt_finish_pixel(a, p, sum);
}

// compact (rank-major, tile-major) -> row-major image
__global__ void pt_untile_kernel(PtRenderArgs a, uint32_t slots_per_rank, const uint8_t* gathered, uint8_t* rgb) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t total = slots_per_rank * a.tile_ranks;
    if (i >= total) return;
    PtRenderArgs r = a;
    r.tile_rank = i / slots_per_rank;
    uint32_t w = i % slots_per_rank, x, y;
    if (!pt_slot_to_pixel(r, w, &x, &y)) return;
    const uint8_t* s = gathered + 3 * (size_t)i;
    uint8_t* d = rgb + 3 * ((size_t)y * a.width + x);
    d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
}

// PORTRAYER_OCC_SEED (tests only, pt_plan_launch): the occluder table filled with hints the test chooses instead of zeros - every entry
// `all` + 1, or entry i = hash(seed, i) mod (n_nodes + 1) (0: none). The table's test is exact whatever an entry holds (pt_trace_packet).
__global__ void __launch_bounds__(256) pt_occ_seed_kernel(uint32_t* __restrict__ occ, uint32_t n, int hashed, uint64_t seed, uint32_t all, uint32_t n_nodes) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    occ[i] = hashed ? (uint32_t)(pt_rng_key(seed, i) % ((uint64_t)n_nodes + 1u)) : all + 1u;
}

// The launch's eye table (PtRenderArgs::eye_tab), one thread per flattened node: the node's `inv` record with its translation column replaced by the camera's eye
// in the node's space - pt_xform_point, the function a lane of the render kernel calls on the same operands (pt_ray_to_local), compiled with the same flags, so
// every entry carries the bits a lane would compute. The primary stage of the mesh-free flat_scene straight-line kernels reads it through the scalar cache
// (pt_test_node_uniform, pt_hit_model). Filled in front of every launch: nothing of it outlives one (the camera moves from frame to frame, so may the nodes).
__global__ void __launch_bounds__(256) pt_eye_table_kernel(const double* __restrict__ inv, double* __restrict__ tab, uint32_t n_nodes, double ex, double ey, double ez) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    const double* m = inv + 12 * (size_t)i;
    double* o = tab + 12 * (size_t)i;
    const PtVec3 e = pt_xform_point(m, pt_v3(ex, ey, ez));
    o[0] = m[0]; o[1] = m[1]; o[2] = m[2]; o[3] = e.x;
    o[4] = m[4]; o[5] = m[5]; o[6] = m[6]; o[7] = e.y;
    o[8] = m[8]; o[9] = m[9]; o[10] = m[10]; o[11] = e.z;
}

// The launch's certain-shadow table (behind the eye table, PtRenderArgs::eye_tab), one thread per flattened node: a ball inside the node's primitive as four floats (pt_certain_ball,
// pt_certain.h). Filled in front of every launch that has an occluder table, like the eye table: pt_scene_update and pt_scene_deform move nodes between launches,
// and two frames in flight have a slot each.
__global__ void __launch_bounds__(256) pt_certain_table_kernel(const uint32_t* __restrict__ info, const double* __restrict__ fwd, const double* __restrict__ inv, float* __restrict__ tab,
                                                               uint32_t n_nodes) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    pt_certain_ball(info[4 * (size_t)i], fwd + 12 * (size_t)i, inv + 12 * (size_t)i, tab + 4 * (size_t)i);
}

#ifndef PT_NO_DARK_LIGHTS
// The launch's dark-light records (in front of the occluder table, PtRenderArgs::occluders; pt_certain.h 4.-8.), behind pt_certain_table_kernel on the launch's stream: a
// block per light, its threads over the nodes' balls. Per light PT_DARK_WORDS words: the lane guard's record {f32(L), ceil} of the LOWEST node whose ball encloses the
// light - all zero where none does - then node + 1 (0: none) and the guard's floor for the tests. Lights x nodes evaluations of a dozen f64 operations each: microseconds
// for the scenes that have an occluder table. Filled in front of every launch like the tables it reads: pt_scene_update moves lights and nodes.
__global__ void __launch_bounds__(256) pt_dark_light_kernel(const double* __restrict__ lights, const float* __restrict__ balls, uint32_t* __restrict__ words, uint32_t n_nodes) {
    __shared__ uint32_t best;
    const double* const light = lights + 15 * (size_t)blockIdx.x;
    if (threadIdx.x == 0) best = 0xFFFFFFFFu;
    __syncthreads();
    float rec[4];
    for (uint32_t i = threadIdx.x; i < n_nodes; i += blockDim.x)
        if (pt_dark_light(light, balls + 4 * (size_t)i, rec)) atomicMin(&best, i);
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint32_t* const o = words + PT_DARK_WORDS * (size_t)blockIdx.x;
    const bool found = best != 0xFFFFFFFFu && pt_dark_light(light, balls + 4 * (size_t)best, rec);
    for (int k = 0; k < 4; k++) o[k] = found ? __builtin_bit_cast(uint32_t, rec[k]) : 0u;
    o[4] = found ? best + 1u : 0u;
    o[5] = found ? __builtin_bit_cast(uint32_t, PT_DARK_D2_MIN) : 0u;
    o[6] = o[7] = 0u;
}
#endif

// The launch's per-pixel candidate lists (pt_pixel_list.h), behind the eye table and the certain-shadow table: a wavefront per 8x8 tile of the launch's own tiles, a lane
// per pixel slot - pixels of partial tiles outside the slice get a record like any other. Which leaves a pixel's beam reaches does not depend on the order in which the
// tree is opened, and pt_pl_insert keeps the K smallest entries and the smallest bound turned away whatever the order of arrival: so the wavefront opens sc.bvh up to 64
// nodes at a time with the TILE's beam (pt_pixel_list.h, 7.: the 8 x 8 rectangle of the tile's slots from lane 0's pixel, whole even where the tile is partial or the launch
// rank-partitioned; wave-uniform, held in scalar registers), in two interleaved phases:
//   1. lanes over nodes. The pending inner nodes are one list per wavefront in LDS. A step pops up to 64 from its end; each lane loads its own node's record with vector
//      loads - all in flight together - and tests both children against the tile's beam. Surviving inner children are appended to the pending list (ballot and lane prefix
//      count), surviving leaf children go to the wavefront's candidate buffer in LDS as {flattened node index, the leaf box's six planes}, one candidate per item of the
//      leaf (sc.bvh_items, resolved by the lane that found it). The dependent round trips per tile are about the tree's levels, not the inner nodes reached.
//   2. lanes over pixels. When the buffer cannot take another step's candidates (PT_PL_STEP_CANDS), or nothing is pending, every lane tests each buffered box - an LDS
//      broadcast, no global load - with its own pixel's beam and inserts what that reaches with the pixel beam's bound. A lane's list is its LDS column, kept sorted
//      (pt_pl_insert); flushing in batches cannot change a record.
// An inner node is pushed once at most, so PT_PL_PENDING words hold any scene of up to 1,024 inner nodes; a pending list that runs full all the same marks the tile's 64
// records "take the walk".
// cap (PORTRAYER_PIXEL_LIST_CAP, tests only): entries a list may hold, <= PT_PL_K. pend_cap (PORTRAYER_PIXEL_LIST_PENDING, tests only): the words of the pending list
// that may be used, 1 .. PT_PL_PENDING - the kernel pops from the end, so on a balanced tree the list stays near 64 x (the levels below the first 64-wide one), a few
// hundred words at 65,536 nodes: the tests of the marked tiles shrink it.
// -DPT_PL_DEPTH_FIRST (make variant; the timing A/B): the kernel this one replaced - one depth-first walk per tile, a node per step through the scalar cache, a node
// entered when any lane's pixel beam reaches it.
// Block size and buffer by measurement (profiles/r13/notes.md section 4): the kernel waits, so what counts is wavefronts per CU, and LDS sets that - a wavefront per block
// and the smallest buffer that takes a step, 9.5 KB a wavefront, 16 wavefronts per CU.
#ifndef PT_PL_DEPTH_FIRST
#define PT_PL_BLOCK 64
#define PT_PL_PENDING 1024u    // words of a wavefront's pending list
#define PT_PL_STEP_CANDS 128u  // the candidates one step can add: 64 nodes x 2 leaf children of one item (direct leaves), or 8 nodes x 2 leaf children x 8 items
#define PT_PL_CANDS 128u       // a wavefront's candidate buffer, 32 bytes each: flushed in front of a step that might not fit - with this size, whenever it holds anything
// (what one lane wrote to LDS, seen by the wavefront's other lanes: same wavefront, program order and a fence suffice)
#define PT_PL_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
static __device__ __forceinline__ float pt_pl_scalar(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); }
static __device__ __forceinline__ uint32_t pt_pl_lanes_below(unsigned long long m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }
__global__ void __launch_bounds__(PT_PL_BLOCK) pt_pixel_list_kernel(PtRenderArgs a, uint32_t* __restrict__ table, uint32_t cap, uint32_t pend_cap, uint32_t flags) {
    __shared__ uint32_t s_list[PT_PL_BLOCK / 64][PT_PL_K][64];
    __shared__ uint32_t s_pend[PT_PL_BLOCK / 64][PT_PL_PENDING];
    __shared__ uint4 s_cand[PT_PL_BLOCK / 64][PT_PL_CANDS * 2u];  // {node, lo.x, lo.y, lo.z}, {hi.x, hi.y, hi.z, -}
    static_assert(PT_PL_CANDS >= PT_PL_STEP_CANDS, "the empty buffer takes a step's candidates");
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t tile_local = PT_UNIFORM_U32(blockIdx.x * (PT_PL_BLOCK / 64) + wave);
    if (tile_local >= a.n_slots / 64u) return;  // (wave-uniform)
    const PtSceneView& sc = a.scene;
    const uint32_t slot = tile_local * 64u + lane;
    uint32_t x, y, tx, ty;
    [[maybe_unused]] const bool inside = pt_slot_to_pixel(a, slot, &x, &y);
    pt_slot_to_pixel(a, tile_local * 64u, &tx, &ty);
#ifndef PT_NO_BACKGROUND_SKIP
    if (tile_local == 0u && lane == 0u) table[-16] = flags;  // header word 0 (the host zeroed the header): what follows it
#endif
    const PtBeam beam = pt_beam_setup(a.cam, (double)x, (double)y);
    PtBeam tile = pt_beam_setup(a.cam, (double)tx, (double)ty, 8.0, 8.0);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        PtBeamAxis& t = tile.ax[k];
        t.neg = __builtin_amdgcn_readfirstlane(t.neg);
        t.a1 = pt_pl_scalar(t.a1); t.a2 = pt_pl_scalar(t.a2); t.be1 = pt_pl_scalar(t.be1); t.be2 = pt_pl_scalar(t.be2); t.bf1 = pt_pl_scalar(t.bf1); t.bf2 = pt_pl_scalar(t.bf2);
    }
    tile.lmin = pt_pl_scalar(tile.lmin);
    uint32_t* const list = &s_list[wave][0][lane];
    uint32_t* const pend = s_pend[wave];
    uint4* const cand = s_cand[wave];
    uint32_t count = 0, tail = PT_PL_INF_BITS;
    if (cap > PT_PL_K) cap = PT_PL_K;  // (the host refuses a larger one; a list's LDS column has PT_PL_K rows)
    if (pend_cap > PT_PL_PENDING) pend_cap = PT_PL_PENDING;
    bool overflowed = false;
    uint32_t n_pend = 0, n_cand = 0;  // (wave-uniform)
    const bool direct = sc.tlas_direct != 0;
    const uint32_t root = sc.tlas_root;
    if (sc.n_nodes != 0 && root != PT_REF_EMPTY) {
        if (root & PT_REF_LEAF) {  // (the walk tests a root leaf without a box test)
            const uint32_t first = (root & ~PT_REF_LEAF) >> 3, n = direct ? 1u : (root & 7u) + 1u;
            for (uint32_t i = 0; i < n; i++) pt_pl_insert(list, 64u, cap, &count, &tail, pt_pl_entry(0.0f, direct ? first : sc.bvh_items[first + i]));
        } else {
            if (lane == 0) pend[0] = root;
            n_pend = 1;
        }
    }
    auto flush = [&]() {  // phase 2
        PT_PL_WAVE_SYNC();
        for (uint32_t j = 0; j < n_cand; j++) {
            const uint4 c0 = cand[2u * j], c1 = cand[2u * j + 1u];
            const float lo[3] = {pt_f32_of(c0.y), pt_f32_of(c0.z), pt_f32_of(c0.w)}, hi[3] = {pt_f32_of(c1.x), pt_f32_of(c1.y), pt_f32_of(c1.z)};
            float bound = 0.0f;
            if (pt_beam_box(beam, lo, hi, &bound)) pt_pl_insert(list, 64u, cap, &count, &tail, pt_pl_entry(bound, c0.x));
        }
        n_cand = 0;
    };
    const uint32_t width = direct ? 64u : PT_PL_STEP_CANDS / 16u;
    while (n_pend > 0) {
        if (n_cand > PT_PL_CANDS - PT_PL_STEP_CANDS) flush();
        PT_PL_WAVE_SYNC();
        // phase 1: a lane per pending node
        const uint32_t take = n_pend < width ? n_pend : width;
        n_pend -= take;
        uint32_t ref[2] = {PT_REF_EMPTY, PT_REF_EMPTY};
        uint32_t nd[12] = {};
        bool reached[2] = {false, false};
        if (lane < take) {
            const uint4* const p = reinterpret_cast<const uint4*>(sc.bvh) + 4u * (size_t)pend[n_pend + lane];  // (PtBvhNode as 16 words: lo[axis][child], hi[axis][child], the children)
            const uint4 q0 = p[0], q1 = p[1], q2 = p[2];
            const uint2 q3 = *reinterpret_cast<const uint2*>(p + 3);
            nd[0] = q0.x; nd[1] = q0.y; nd[2] = q0.z; nd[3] = q0.w; nd[4] = q1.x; nd[5] = q1.y; nd[6] = q1.z; nd[7] = q1.w; nd[8] = q2.x; nd[9] = q2.y; nd[10] = q2.z; nd[11] = q2.w;
            ref[0] = q3.x; ref[1] = q3.y;
#pragma unroll
            for (int ch = 0; ch < 2; ch++) {
                if (ref[ch] == PT_REF_EMPTY) continue;
                float lo[3], hi[3], bound;
#pragma unroll
                for (int k = 0; k < 3; k++) { lo[k] = pt_f32_of(nd[2 * k + ch]); hi[k] = pt_f32_of(nd[6 + 2 * k + ch]); }
                reached[ch] = pt_beam_box(tile, lo, hi, &bound);
            }
        }
        const bool inner0 = reached[0] && !(ref[0] & PT_REF_LEAF), inner1 = reached[1] && !(ref[1] & PT_REF_LEAF);
        const unsigned long long m0 = __ballot(inner0), m1 = __ballot(inner1);
        const uint32_t n0 = (uint32_t)__builtin_popcountll(m0), n1 = (uint32_t)__builtin_popcountll(m1);
        if (n_pend + n0 + n1 > pend_cap) { overflowed = true; break; }
        if (inner0) pend[n_pend + pt_pl_lanes_below(m0)] = ref[0];
        if (inner1) pend[n_pend + n0 + pt_pl_lanes_below(m1)] = ref[1];
        n_pend += n0 + n1;
#pragma unroll
        for (int ch = 0; ch < 2; ch++) {
            const bool leaf = reached[ch] && (ref[ch] & PT_REF_LEAF);
            const uint32_t first = (ref[ch] & ~PT_REF_LEAF) >> 3, n = !leaf ? 0u : (direct ? 1u : (ref[ch] & 7u) + 1u);
            for (uint32_t i = 0; i < 8u; i++) {
                const bool mine = i < n;
                const unsigned long long m = __ballot(mine);
                if (m == 0) break;
                if (mine) {
                    const uint32_t at = 2u * (n_cand + pt_pl_lanes_below(m));
                    cand[at] = make_uint4(direct ? first : sc.bvh_items[first + i], nd[ch], nd[2 + ch], nd[4 + ch]);
                    cand[at + 1u] = make_uint4(nd[6 + ch], nd[8 + ch], nd[10 + ch], 0u);
                }
                n_cand += (uint32_t)__builtin_popcountll(m);
            }
        }
    }
    if (!overflowed && n_cand) flush();
    // (each lane its own record, 16-byte stores a record apart: staging the tile's records in LDS and storing them by rows was measured and gained nothing -
    // profiles/r13/notes.md section 4)
    uint32_t* rec = table + (size_t)slot * PT_PL_WORDS;
    uint32_t wds[PT_PL_WORDS];
    wds[0] = overflowed ? PT_PL_WALK : count;
    wds[1] = tail;
#pragma unroll
    for (uint32_t k = 0; k < PT_PL_K; k++) wds[2 + k] = k < count ? list[k * 64u] : 0u;
#pragma unroll
    for (uint32_t k = 2 + PT_PL_K; k < PT_PL_WORDS; k++) wds[k] = 0u;
#pragma unroll
    for (uint32_t k = 0; k < PT_PL_WORDS; k += 4) reinterpret_cast<uint4*>(rec)[k / 4] = make_uint4(wds[k], wds[k + 1], wds[k + 2], wds[k + 3]);
#ifndef PT_NO_BACKGROUND_SKIP
    // The queue (pt_pixel_list.h): the tile's pixels that need the render kernel - inside the slice, and not {no entry, nothing left out, unmarked} - as one 64-bit mask
    // per tile behind the queue's array, bit L for the pixel the render kernel deals L-th in the tile (pt_tile_order_to_slot). pt_pixel_queue_kernel makes the queue of them.
    if (flags & PT_PL_QUEUE) {
        const bool needed = inside && (overflowed || count != 0u || tail != PT_PL_INF_BITS);
        const bool mine = __shfl((int)needed, (int)pt_tile_order_to_slot(lane)) != 0;
        const unsigned long long m = __ballot(mine);
        if (lane == 0) pt_pl_masks(table, a.n_slots)[tile_local] = m;
    }
#endif
}

#ifndef PT_NO_BACKGROUND_SKIP
// The queue from the tiles' masks, behind the list kernel on the launch's stream: a block per 256 tiles. The tiles' ranges lie in the order of the tiles - the order the
// items were dealt in before there was a queue, so that a tile is still rendered well behind the one above it, whose occluder-table entries it starts from
// (pt_trace_packet: PtOccRef::back) - and inside a range the ids go in the tile's Morton order. Every block adds up the masks in front of its own tiles for itself
// (a 1080p launch has 32,400 of them, 8 bytes each, in the cache): no second launch for a scan, no waiting of block on block. The last block leaves the length in header word 1.
__global__ void __launch_bounds__(256) pt_pixel_queue_kernel(uint32_t* __restrict__ table, uint32_t n_slots) {
    __shared__ uint32_t part[256];
    __shared__ uint32_t offs[256];
    const uint32_t tiles = n_slots / 64u, first = blockIdx.x * 256u, t = threadIdx.x, lane = t & 63u;
    const unsigned long long* const masks = pt_pl_masks(table, n_slots);
    uint32_t* const queue = table + (size_t)n_slots * PT_PL_WORDS;
    uint32_t before = 0, i = t;
    for (; i + 7u * 256u < first; i += 8u * 256u) {  // (eight loads in flight: taken one by one, the last block's 126 round trips were most of the kernel's 47 us)
        unsigned long long v[8];
#pragma unroll
        for (uint32_t k = 0; k < 8u; k++) v[k] = masks[i + k * 256u];
#pragma unroll
        for (uint32_t k = 0; k < 8u; k++) before += (uint32_t)__builtin_popcountll(v[k]);
    }
    for (; i < first; i += 256u) before += (uint32_t)__builtin_popcountll(masks[i]);
    const unsigned long long mine = first + t < tiles ? masks[first + t] : 0ull;
    part[t] = before; offs[t] = (uint32_t)__builtin_popcountll(mine);
    __syncthreads();
    for (uint32_t s = 128u; s > 0u; s >>= 1) {  // the sum of what lies in front of the block
        if (t < s) part[t] += part[t + s];
        __syncthreads();
    }
    const uint32_t base = part[0];
    for (uint32_t s = 1u; s < 256u; s <<= 1) {  // inclusive scan of the block's own counts
        const uint32_t v = t >= s ? offs[t - s] : 0u;
        __syncthreads();
        offs[t] += v;
        __syncthreads();
    }
    if (first + 256u >= tiles && t == 255u) table[-15] = base + offs[255];  // (the tiles behind the launch's last count nothing)
    for (uint32_t k = 0; k < 64u; k++) {  // a wavefront per tile, 64 tiles each: lane L is the tile's L-th pixel in Morton order
        const uint32_t i = (t & ~63u) + k, tile = first + i;
        if (tile >= tiles) break;  // (wave-uniform)
        const unsigned long long m = (unsigned long long)__shfl((long long)mine, (int)k);  // (thread i of the block read tile i's mask: lane k of this wavefront)
        const uint32_t at = base + (i ? offs[i - 1u] : 0u) + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
        if (((m >> lane) & 1ull) && at < n_slots) queue[at] = (tile << 6) | pt_tile_order_to_slot(lane);  // (a slot is queued once at most: the bound always holds)
    }
}
#endif
#else
#define PT_PL_BLOCK 256
#define PT_PL_STACK 64
__global__ void __launch_bounds__(PT_PL_BLOCK) pt_pixel_list_kernel(PtRenderArgs a, uint32_t* __restrict__ table, uint32_t cap, uint32_t pend_cap, uint32_t flags) {
    __shared__ uint32_t s_list[PT_PL_BLOCK / 64][PT_PL_K][64];
    __shared__ uint32_t s_stack[PT_PL_BLOCK / 64][PT_PL_STACK];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t tile_local = blockIdx.x * (PT_PL_BLOCK / 64) + wave;
    if (tile_local >= a.n_slots / 64u) return;  // (wave-uniform)
#ifndef PT_NO_BACKGROUND_SKIP
    if (tile_local == 0u && lane == 0u) table[-16] = flags;  // header word 0 (the host never asks this variant for a queue)
#endif
    const PtSceneView& sc = a.scene;
    const uint32_t slot = tile_local * 64u + lane;
    uint32_t x, y;
    pt_slot_to_pixel(a, slot, &x, &y);
    const PtBeam beam = pt_beam_setup(a.cam, (double)x, (double)y);
    uint32_t* const list = &s_list[wave][0][lane];
    uint32_t* const stack = s_stack[wave];
    uint32_t count = 0, tail = PT_PL_INF_BITS;
    if (cap > PT_PL_K) cap = PT_PL_K;  // (the host refuses a larger one; a list's LDS column has PT_PL_K rows)
    bool overflowed = false;
    int sp = 0;
    auto add_leaf = [&](uint32_t ref, bool reached, float bound) {  // ref: a leaf reference (wave-uniform)
        const uint32_t first = (ref & ~PT_REF_LEAF) >> 3, n = (ref & 7u) + 1u;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t node = sc.tlas_direct ? first : sc.bvh_items[first + i];
            if (reached) pt_pl_insert(list, 64u, cap, &count, &tail, pt_pl_entry(bound, node));
        }
    };
    const uint32_t root = sc.tlas_root;
    if (sc.n_nodes != 0 && root != PT_REF_EMPTY) {
        if (root & PT_REF_LEAF) add_leaf(root, true, 0.0f);  // (the walk tests a root leaf without a box test)
        else { stack[0] = root; sp = 1; }
    }
    while (sp > 0) {
        // (lane 0's pushes of the step before, seen by the whole wavefront: same wavefront, program order and a fence suffice)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint32_t cur = (uint32_t)__builtin_amdgcn_readfirstlane((int)stack[sp - 1]);
        sp--;
        const pt_u32x16 nd = pt_sload_node(sc.bvh, cur);  // (PtBvhNode as 16 words in scalar registers, as the render kernel's walk fetches it: lo[axis][child], hi[axis][child], the children)
#pragma unroll
        for (int ch = 0; ch < 2; ch++) {
            const uint32_t ref = nd[12 + ch];
            if (ref == PT_REF_EMPTY) continue;
            float lo[3], hi[3], bound = 0.0f;
#pragma unroll
            for (int k = 0; k < 3; k++) { lo[k] = pt_f32_of(nd[2 * k + ch]); hi[k] = pt_f32_of(nd[6 + 2 * k + ch]); }
            const bool reached = pt_beam_box(beam, lo, hi, &bound);
            if (!__any(reached)) continue;
            if (ref & PT_REF_LEAF) add_leaf(ref, reached, bound);
            else if (sp < PT_PL_STACK) { if (lane == 0) stack[sp] = ref; sp++; }
            else overflowed = true;
        }
    }
    uint32_t* rec = table + (size_t)slot * PT_PL_WORDS;
    uint32_t wds[PT_PL_WORDS];
    wds[0] = overflowed ? PT_PL_WALK : count;
    wds[1] = tail;
#pragma unroll
    for (uint32_t k = 0; k < PT_PL_K; k++) wds[2 + k] = k < count ? list[k * 64u] : 0u;
#pragma unroll
    for (uint32_t k = 0; k < PT_PL_WORDS; k += 4) reinterpret_cast<uint4*>(rec)[k / 4] = make_uint4(wds[k], wds[k + 1], wds[k + 2], wds[k + 3]);
}
#endif

// ------------------------------------------------------------------------------------------------
// The life of a device pass (PtPass), the same for every kind. Queueing: prepare, [the kind's argument block and sizing dispatch], open, [its sort and kernels],
// seal. On the pass's stream that is: all of misc zeroed, ev0, the sort and the kernels, ev1, the overflow flag's copy to the pinned page, copy_done.
// Closing: wait, result. The entry points: pt_pass_device_tail ... pt_pass_finish, or pt_pass_settle ... pt_pass_result within one call (host buffers).
// ------------------------------------------------------------------------------------------------
#define PT_PASS_MISC_BYTES (256 + PT_FINE_QUEUES * PT_QUEUE_STRIDE * 4)
static size_t pt_stack_column(const PtSceneView& sc, int stack_lds_cap);

// The events and the pinned page, made by the pass's first use: a context that never runs the pass never pays for them.
static int pt_pass_prepare(pt_context* c, PtPass& v) {
    if (v.ev0) return PT_OK;
    PT_HIP(c, hipEventCreate(&v.ev0));
    PT_HIP(c, hipEventCreate(&v.ev1));
    PT_HIP(c, hipEventCreateWithFlags(&v.copy_done, hipEventDisableTiming));
    PT_HIP(c, hipHostMalloc((void**)&v.host, 256, hipHostMallocDefault));
    return PT_OK;
}

// The work buffers for a launch of `grid` blocks (the sizing dispatch's figure, with r.stack_lds_cap set) and `r` pointed into them; then misc zeroed and the first
// event on `stream`. frames: the kernels keep recursion frames (the interpreter's). The items come one at a time from 16 interleaved queues, as a render of this
// size has them (pt_plan_launch).
static int pt_pass_open(pt_context* c, PtPass& v, PtRenderArgs& r, uint32_t grid, bool frames, hipStream_t stream) {
    r.n_lanes = grid * PT_BLOCK;
    int rc;
    if ((rc = pt_reserve(c, v.stack_spill, (size_t)r.n_lanes * pt_stack_column(r.scene, r.stack_lds_cap) * 4))) return rc;
    if (frames && (rc = pt_reserve(c, v.spill, pt_needs_spill(c->traits) ? (size_t)r.n_lanes * PT_SPILL_DEPTHS * PT_SPILL_STRIDE * sizeof(double) : 16))) return rc;
    if ((rc = pt_reserve(c, v.misc, PT_PASS_MISC_BYTES))) return rc;
    r.stack_spill = (uint32_t*)v.stack_spill.p;
    if (frames) r.spill = (double*)v.spill.p;
    r.overflow_flag = (unsigned int*)v.misc.p + 1;
    r.work_queues = (unsigned int*)((char*)v.misc.p + 256);
    r.fine_queues = 16;
    v.stream = stream; v.queued = true; v.closed = false;  // from here on something of the pass may be in flight on `stream`, whatever fails below
    PT_HIP(c, hipMemsetAsync(v.misc.p, 0, PT_PASS_MISC_BYTES, stream));
    PT_HIP(c, hipEventRecord(v.ev0, stream));
    return PT_OK;
}

// Behind the kernels: the second event, and the overflow flag on its way to the pinned page.
static int pt_pass_seal(pt_context* c, PtPass& v) {
    PT_HIP(c, hipEventRecord(v.ev1, v.stream));
    PT_HIP(c, hipMemcpyAsync(v.host, v.misc.p, 8, hipMemcpyDeviceToHost, v.stream));
    PT_HIP(c, hipEventRecord(v.copy_done, v.stream));
    v.closed = true;
    return PT_OK;
}

// Waits for whatever the last queueing left in flight: the event behind its last copy, or - where queueing failed half way - its stream.
static int pt_pass_wait(pt_context* c, PtPass& v) {
    if (!v.queued) return PT_OK;
    v.queued = false;
    if (v.closed) PT_HIP(c, hipEventSynchronize(v.copy_done));
    else PT_HIP(c, hipStreamSynchronize(v.stream));
    return PT_OK;
}

// After the pass's copy_done: the kernel time and what the overflow flag says (as pt_collect_stats reads a render's).
static int pt_pass_result(pt_context* c, PtPass& v, double* kernel_ms) {
    unsigned int head[2];
    memcpy(head, v.host, sizeof head);
    if (kernel_ms) {
        float ms = 0.f;
        PT_HIP(c, hipEventElapsedTime(&ms, v.ev0, v.ev1));
        *kernel_ms = ms;
    }
    if (head[1] & 4u) return pt_fail(c, PT_ERR_TRAVERSAL, "a tree walk did not end (watchdog): results invalid");
    if (head[1]) return pt_fail(c, PT_ERR_TRAVERSAL, "traversal stack overflow");
    return PT_OK;
}

// The end of a _device entry point; rc: what queueing returned. What was queued before a failure must not outlive the call: the next pass may reallocate the
// buffers under it.
static int pt_pass_device_tail(pt_context* c, PtPass& v, int rc) {
    if (rc) { pt_pass_wait(c, v); return rc; }
    v.pending = true;
    return PT_OK;
}
// ... and the middle of a host-buffer one, in front of its copies back: it waits whether or not queueing failed, and the queueing error comes first.
static int pt_pass_settle(pt_context* c, PtPass& v, int rc) {
    const int rc_wait = pt_pass_wait(c, v);
    return rc ? rc : rc_wait;
}

// The staging of a host-buffer entry point, the same for every kind: a table with a row per array of the caller's and the PtBuf that holds its device copy.
// A row whose host pointer is null is absent: an output not asked for, an optional input not given.
struct PtStage {
    const void* in;  // the caller's array that goes to the device in front of the pass ...
    void* out;       // ... or the one that comes back behind it
    PtBuf* buf;
    size_t bytes;
    void* dev;       // buf's memory once pt_stage_in has reserved it; null for an absent row
};
static PtStage pt_stage_input(const void* host, PtBuf& buf, size_t bytes) { return {host, nullptr, &buf, bytes, nullptr}; }
static PtStage pt_stage_output(void* host, PtBuf& buf, size_t bytes) { return {nullptr, host, &buf, bytes, nullptr}; }

// In front of the kind's _common: every row's PtBuf reserved, in the table's order, then the inputs copied in.
template <int N>
static int pt_stage_in(pt_context* c, PtStage (&rows)[N]) {
    for (PtStage& s : rows) {
        if (!s.in && !s.out) continue;
        if (int rc = pt_reserve(c, *s.buf, s.bytes)) return rc;
        s.dev = s.buf->p;
    }
    for (PtStage& s : rows)
        if (s.in && s.bytes) PT_HIP(c, hipMemcpy(s.dev, s.in, s.bytes, hipMemcpyHostToDevice));
    return PT_OK;
}

// Behind it; rc: what queueing returned. The pass settled (pt_pass_settle), then the outputs copied back, then the pass's result. window (pt_aov, pt_guides):
// the rows are images of window's size and only its slice's rectangle comes back (the kernel wrote nothing else, and the device copies hold nothing else of
// value): picking one pixel of a 1920x1080 frame moves 68 bytes, and pixels outside the slice keep the caller's bytes because they are never touched.
template <int N>
static int pt_stage_out(pt_context* c, PtPass& v, int rc, PtStage (&rows)[N], double* kernel_ms, const pt_aov_params* window = nullptr) {
    if ((rc = pt_pass_settle(c, v, rc))) return rc;
    for (PtStage& s : rows) {
        if (!s.out) continue;
        if (!window) { PT_HIP(c, hipMemcpy(s.out, s.dev, s.bytes, hipMemcpyDeviceToHost)); continue; }
        const pt_rect& sl = window->slice;
        if (sl.x1 < sl.x0 || sl.y1 < sl.y0) break;
        const size_t elem = s.bytes / ((size_t)window->width * window->height), cols = (size_t)sl.x1 - sl.x0 + 1, lines = (size_t)sl.y1 - sl.y0 + 1;
        const size_t pitch = (size_t)window->width * elem, first = ((size_t)sl.y0 * window->width + sl.x0) * elem;
        PT_HIP(c, hipMemcpy2D((char*)s.out + first, pitch, (const char*)s.dev + first, pitch, cols * elem, lines, hipMemcpyDeviceToHost));
    }
    return pt_pass_result(c, v, kernel_ms);
}

// A _finish entry point (c is not NULL); none: what it says when no _device call of the pass is open.
static int pt_pass_finish(pt_context* c, PtPass& v, const char* none, double* kernel_ms) {
    if (!v.pending) return pt_fail(c, PT_ERR_ARGUMENT, none);
    PT_HIP(c, hipSetDevice(c->device));
    v.pending = false;
    int rc = pt_pass_wait(c, v);
    if (rc) return rc;
    return pt_pass_result(c, v, kernel_ms);
}

// pt_context_destroy, behind the pass's wait: what is not a PtBuf.
static void pt_pass_release(PtPass& v) {
    if (v.ev0) hipEventDestroy(v.ev0);
    if (v.ev1) hipEventDestroy(v.ev1);
    if (v.copy_done) hipEventDestroy(v.copy_done);
    if (v.host) hipHostFree(v.host);
}

extern "C" int pt_abi_version(void) { return PT_ABI_VERSION; }

extern "C" int pt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int pt_context_create(int device, pt_context** out) {
    if (!out) return PT_ERR_ARGUMENT;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return PT_ERR_DEVICE;
    pt_context* c = new pt_context();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess) { delete c; return PT_ERR_DEVICE; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { delete c; return PT_ERR_DEVICE; }
    c->n_cu = prop.multiProcessorCount;
    for (auto& sl : c->slot)
        if (hipEventCreate(&sl.ev0) != hipSuccess || hipEventCreate(&sl.ev1) != hipSuccess || hipEventCreateWithFlags(&sl.copy_done, hipEventDisableTiming) != hipSuccess ||
            hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking) != hipSuccess ||
            hipHostMalloc((void**)&sl.host, PT_SLOT_BYTES, hipHostMallocDefault) != hipSuccess) {
            pt_context_destroy(c);
            return PT_ERR_DEVICE;
        }
    memset(&c->view, 0, sizeof c->view);
    *out = c;
    return PT_OK;
}

extern "C" void pt_context_destroy(pt_context* c) {
    if (!c) return;
    hipSetDevice(c->device);
    // Whatever a pass or a render still has in flight may read any buffer of the context: all of it is waited for before anything is freed.
    for (PtPass* v : c->passes) pt_pass_wait(c, *v);
    for (auto& sl : c->slot) {
        if (sl.pending) hipEventSynchronize(sl.copy_done);
        if (sl.stream) hipStreamSynchronize(sl.stream);
    }
    for (pt_film* f : c->films) delete f;
    for (PtPass* v : c->passes) pt_pass_release(*v);
    for (auto& sl : c->slot) {
        if (sl.stream) hipStreamDestroy(sl.stream);
        if (sl.ev0) hipEventDestroy(sl.ev0);
        if (sl.ev1) hipEventDestroy(sl.ev1);
        if (sl.copy_done) hipEventDestroy(sl.copy_done);
        if (sl.host) hipHostFree(sl.host);
    }
    delete c;  // (with every PtBuf it holds)
}

extern "C" const char* pt_last_error(const pt_context* c) { return c ? c->err.c_str() : "no context"; }

// The context's own stream for the render that takes slot `slot & 1` (the slots are taken in turn: 0, 1, 0, ..): a caller that hands consecutive frames to
// pt_render_device on pt_context_stream(ctx, k & 1) lets frame k + 1 start on the wavefront slots frame k's tail frees (see pt_context::Slot).
// Scenes that park recursion frames in HBM (reflective materials: the chain and interpreter kernels) get ONE stream for both slots: two of their launches at
// once double the frames' working set (277 MB per launch at full occupancy) past what the memory-side cache holds - measured: the mirror scene 18.8 -> 19.6 ms
// per frame with two streams, where big-scene's share of an 8-way split gains 2.4 % and macho-cows 1.5 % (profiles/r05/c12_overlap.txt).
// PORTRAYER_TWO_STREAMS=0 / 1 forces one / two.
extern "C" void* pt_context_stream(pt_context* c, int slot) {
    if (!c) return nullptr;
    const bool two = pt_env_on("PORTRAYER_TWO_STREAMS", !(c->have_scene && pt_needs_spill(c->traits)));
    return (void*)c->slot[two ? (slot & 1) : 0].stream;
}
extern "C" int pt_context_next_slot(const pt_context* c) { return c ? c->slot_next : 0; }

// ------------------------------------------------------------------------------------------------
// Render
// ------------------------------------------------------------------------------------------------
static uint32_t pt_slots_per_rank(const pt_render_params* p) {
    uint32_t rw = p->slice.x1 - p->slice.x0 + 1, rh = p->slice.y1 - p->slice.y0 + 1;
    uint32_t tiles = ((rw + 7) / 8) * ((rh + 7) / 8);
    uint32_t ranks = p->tile_ranks ? p->tile_ranks : 1;
    return ((tiles + ranks - 1) / ranks) * 64;
}

extern "C" uint64_t pt_compact_bytes(const pt_render_params* p) {
    if (!p || p->slice.x1 < p->slice.x0 || p->slice.y1 < p->slice.y0) return 0;
    return 3ull * pt_slots_per_rank(p);
}

static int pt_check_params(pt_context* c, const pt_camera* cam, const pt_render_params* p) {
    if (!c || !cam || !p) return PT_ERR_ARGUMENT;
    if (!c->have_scene) return pt_fail(c, PT_ERR_NO_SCENE, "no scene uploaded");
    if (p->width == 0 || p->height == 0 || p->samples == 0) return pt_fail(c, PT_ERR_ARGUMENT, "width, height and samples must be positive");
    if (p->slice.x0 >= p->width || p->slice.x1 >= p->width || p->slice.y0 >= p->height || p->slice.y1 >= p->height)
        return pt_fail(c, PT_ERR_SLICE, "slice corner outside the image (render.rs:79-90)");
    if (p->tile_ranks == 0 || p->tile_rank >= p->tile_ranks) return pt_fail(c, PT_ERR_ARGUMENT, "tile_rank must be < tile_ranks");
    if (p->sample_mode != PT_SAMPLE_CENTRE && p->sample_mode != PT_SAMPLE_RNG) return pt_fail(c, PT_ERR_ARGUMENT, "bad sample_mode");
    // work items of one launch are indexed in 32 bits (pixel slots x 8-sample chunks): refuse what would wrap
    if (!(p->slice.x1 < p->slice.x0 || p->slice.y1 < p->slice.y0)) {
        uint64_t work = (uint64_t)pt_slots_per_rank(p) * ((p->samples + PT_SAMPLE_CHUNK - 1) / PT_SAMPLE_CHUNK);
        if (work >= 0xFFFFFFFFull - 65536)
            return pt_fail(c, PT_ERR_ARGUMENT, "slice x samples too large for one launch (pixel slots x ceil(samples / 8) must stay below 2^32): render it in slices");
    }
    return PT_OK;
}

// a.run_variant (PT_RUN_*, pt_render_kernel.h) selects the kernel.
static hipError_t pt_dispatch(const PtRenderArgs& a, bool stats, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    const bool tex = a.scene.mat_maps != nullptr;
    PT_MODE_LAUNCH(pt_launch_mode_, a.scene.mode, a, a.run_variant, stats, tex, n_cu, stream, grid, launch)
}

// The part of the kernel arguments that follows from the render parameters alone: the slice, the rank's tiles, how a wavefront's
// 64 lanes are laid over pixels x chunks x samples, and the number of work items (pt_shade.h: pt_item_lane).
static void pt_fill_work(const pt_render_params* p, PtRenderArgs* a) {
    a->background_rows = p->background_rows;
    a->width = p->width; a->height = p->height;
    a->x0 = p->slice.x0; a->y0 = p->slice.y0; a->x1 = p->slice.x1; a->y1 = p->slice.y1;
    a->samples = p->samples; a->seed = p->seed; a->jitter_mode = p->sample_mode;
    a->tile_rank = p->tile_rank; a->tile_ranks = p->tile_ranks;
    bool empty = p->slice.x1 < p->slice.x0 || p->slice.y1 < p->slice.y0;  // render.rs:60-65: an inverted slice renders nothing
    a->n_slots = empty ? 0 : pt_slots_per_rank(p);
    a->n_chunks = (p->samples + PT_SAMPLE_CHUNK - 1) / PT_SAMPLE_CHUNK;
    // K samples of a pixel run side by side in a wavefront: a whole chunk from SAMPLES = 8 on, else the next power of two
    uint32_t k = PT_SAMPLE_CHUNK;
    if (p->samples < PT_SAMPLE_CHUNK) { k = 1; while (k < p->samples) k *= 2; }
    a->lane_samples = k;
    // C chunks of a pixel side by side: the largest of 8, 4, 2, 1 that leaves at most 1/16 of the chunk slots empty
    // (SAMPLES = 64: 8 chunks -> C = 8, one pixel per wavefront; SAMPLES = 16: C = 2; SAMPLES = 100, 13 chunks: C = 1)
    uint32_t cc = 1;
    if (k == PT_SAMPLE_CHUNK)
        for (uint32_t cand = 8; cand > 1; cand /= 2) {
            uint32_t slots = (a->n_chunks + cand - 1) / cand * cand;
            if ((slots - a->n_chunks) * 16 <= a->n_chunks) { cc = cand; break; }
        }
    if (const char* e = getenv("PORTRAYER_LANE_CHUNKS")) { uint32_t v = (uint32_t)atoi(e); if (k == PT_SAMPLE_CHUNK && (v == 1 || v == 2 || v == 4 || v == 8)) cc = v; }
    a->lane_chunks = cc;
    a->n_items = (a->n_slots / 64) * ((a->n_chunks + cc - 1) / cc) * (k * cc);
    for (a->k_log2 = 0; (1u << a->k_log2) < k; a->k_log2++) { }
    for (a->c_log2 = 0; (1u << a->c_log2) < cc; a->c_log2++) { }
    a->div_groups = pt_fastdiv_make((a->n_chunks + cc - 1) / cc);
    a->div_tiles_x = pt_fastdiv_make(empty ? 1u : (p->slice.x1 - p->slice.x0 + 1u + 7u) / 8u);
}

static int pt_fill_args(pt_context* c, const pt_camera* cam, const pt_render_params* p, PtRenderArgs* a) {
    memset(a, 0, sizeof *a);
    a->scene = c->view;
    for (int k = 0; k < 3; k++) a->cam.eye[k] = cam->eye[k];
    for (int k = 0; k < 12; k++) a->cam.view_to_world[k] = cam->view_to_world[k];
    a->cam.fov_factor = cam->fov_factor; a->cam.aspect = cam->aspect_ratio; a->cam.width = cam->width; a->cam.height = cam->height;
    pt_fill_work(p, a);
    return PT_OK;
}

// Host-side replay of the kernel's work decomposition (no GPU involved): every work item of a launch with these parameters,
// every lane of it, through the same pt_item_lane the kernel uses. Per pixel of the image: how many (lane, item) pairs carry a
// sample of it, the sum of their sample indices, and the sum of the chunk lengths reported by the lanes that add a chunk up.
// Tests check that every sample of every pixel of the rank's tiles is covered exactly once.
extern "C" int pt_test_work_items(const pt_render_params* p, uint32_t* sample_count, uint64_t* sample_index_sum, uint32_t* chunk_length_sum,
                                  uint64_t* n_items, uint32_t* lane_pixels_chunks_samples) {
    if (!p || !sample_count || !sample_index_sum || !chunk_length_sum) return PT_ERR_ARGUMENT;
    if (p->width == 0 || p->height == 0 || p->samples == 0 || p->tile_ranks == 0 || p->tile_rank >= p->tile_ranks) return PT_ERR_ARGUMENT;
    if (p->slice.x0 >= p->width || p->slice.x1 >= p->width || p->slice.y0 >= p->height || p->slice.y1 >= p->height) return PT_ERR_SLICE;
    PtRenderArgs a;
    memset(&a, 0, sizeof a);
    pt_fill_work(p, &a);
    if (n_items) *n_items = a.n_items;
    if (lane_pixels_chunks_samples) {
        lane_pixels_chunks_samples[0] = 64u / (a.lane_samples * a.lane_chunks); lane_pixels_chunks_samples[1] = a.lane_chunks; lane_pixels_chunks_samples[2] = a.lane_samples;
    }
    for (uint32_t w = 0; w < a.n_items; w++)
        for (uint32_t lane = 0; lane < 64; lane++) {
            PtItemLane it, it_k;
            uint32_t x, y, x_k, y_k;
            const bool mine = pt_item_lane(a, w, lane, &it, &x, &y);
            // what the render kernels actually run (shifts + multiply-high divisions) must agree in every field
            const bool mine_k = pt_item_lane_fast(a, w, lane, &it_k, &x_k, &y_k);
            if (mine != mine_k || it.slot != it_k.slot || it.chunk != it_k.chunk || it.sample != it_k.sample || it.first != it_k.first || it.count != it_k.count ||
                (mine && (x != x_k || y != y_k)))
                return PT_ERR_TRAVERSAL;
            if (!mine) continue;
            if (x >= p->width || y >= p->height) return PT_ERR_TRAVERSAL;  // would write outside the image
            const size_t px = (size_t)y * p->width + x;
            sample_count[px]++;
            sample_index_sum[px] += it.sample;
            if (it.first) chunk_length_sum[px] += it.count;
        }
    return PT_OK;
}

// Host-side run (no GPU involved) of the walks' f32 slab test: pair i is ray i (origins / directions: 3 doubles each, range [0, t_max[i]]) against box i
// (box_lo / box_hi: 3 floats each). body 0: the constants the kernels are built with (pt_raypk), 1: the f64-product body, 2: the f32 body.
// Out per pair: t_near / t_far = the interval of the per-lane form (pt_slab_seg_pk's expressions: entering clamped at 0, leaving at the rounded t_max) and
// verdict, bit 0: pt_slab_seg_pk accepts, bit 1: pt_slab_pk2<PT_OCT_MIXED> accepts (the box as both children), bit 2: pt_slab_pk2 under the ray's own octant
// accepts (a ray with a switched-off axis has no octant: bit 2 repeats bit 1), bit 3: the two children of either form disagree. Tests check that a box the
// exact ray meets is never rejected.
extern "C" int pt_test_raypk(uint64_t n, int body, const double* origins, const double* directions, const double* t_max, const float* box_lo, const float* box_hi,
                             int32_t* verdict, float* t_near, float* t_far) {
    if (!origins || !directions || !t_max || !box_lo || !box_hi || !verdict || !t_near || !t_far || body < 0 || body > 2) return PT_ERR_ARGUMENT;
    for (uint64_t i = 0; i < n; i++) {
        PtRay r;
        r.o = pt_v3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]);
        r.d = pt_v3(directions[3 * i], directions[3 * i + 1], directions[3 * i + 2]);
        PtRayPk q;
        int s[3];
        if (body == 0) {  // (what pt_raypk(r) does)
            s[0] = pt_raypk_axis(r.o.x, r.d.x, &q.a[0], &q.b[0]); s[1] = pt_raypk_axis(r.o.y, r.d.y, &q.a[1], &q.b[1]); s[2] = pt_raypk_axis(r.o.z, r.d.z, &q.a[2], &q.b[2]);
        } else if (body == 1) {
            s[0] = pt_raypk_axis_f64(r.o.x, r.d.x, &q.a[0], &q.b[0]); s[1] = pt_raypk_axis_f64(r.o.y, r.d.y, &q.a[1], &q.b[1]); s[2] = pt_raypk_axis_f64(r.o.z, r.d.z, &q.a[2], &q.b[2]);
        } else {
            s[0] = pt_raypk_axis_f32(r.o.x, r.d.x, &q.a[0], &q.b[0]); s[1] = pt_raypk_axis_f32(r.o.y, r.d.y, &q.a[1], &q.b[1]); s[2] = pt_raypk_axis_f32(r.o.z, r.d.z, &q.a[2], &q.b[2]);
        }
        const float* lo = box_lo + 3 * i;
        const float* hi = box_hi + 3 * i;
        const float tm = pt_tmax32(t_max[i]);
        const float ax = __builtin_fmaf(lo[0], q.a[0].x, q.a[0].y), bx = __builtin_fmaf(hi[0], q.b[0].x, q.b[0].y);
        const float ay = __builtin_fmaf(lo[1], q.a[1].x, q.a[1].y), by = __builtin_fmaf(hi[1], q.b[1].x, q.b[1].y);
        const float az = __builtin_fmaf(lo[2], q.a[2].x, q.a[2].y), bz = __builtin_fmaf(hi[2], q.b[2].x, q.b[2].y);
        t_near[i] = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), 0.0f));
        t_far[i] = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fminf(fmaxf(az, bz), tm));
        int v = pt_slab_seg_pk(lo, hi, q, 0.0f, tm) ? 1 : 0;
        pt_u32x16 rec;
        for (int k = 0; k < 16; k++) rec[k] = 0u;
        for (int k = 0; k < 3; k++) {
            uint32_t l, h;
            memcpy(&l, lo + k, 4); memcpy(&h, hi + k, 4);
            rec[2 * k] = rec[2 * k + 1] = l; rec[6 + 2 * k] = rec[6 + 2 * k + 1] = h;
        }
        unsigned long long m0 = 0, m1 = 0, first = 0, o0 = 0, o1 = 0;
        pt_slab_pk2<PT_OCT_MIXED>(rec, q, tm, &m0, &m1, &first);
        o0 = m0; o1 = m1;
        if (s[0] && s[1] && s[2]) {
            switch ((s[0] == 2 ? 1 : 0) | (s[1] == 2 ? 2 : 0) | (s[2] == 2 ? 4 : 0)) {
                case 0: pt_slab_pk2<0>(rec, q, tm, &o0, &o1, &first); break;
                case 1: pt_slab_pk2<1>(rec, q, tm, &o0, &o1, &first); break;
                case 2: pt_slab_pk2<2>(rec, q, tm, &o0, &o1, &first); break;
                case 3: pt_slab_pk2<3>(rec, q, tm, &o0, &o1, &first); break;
                case 4: pt_slab_pk2<4>(rec, q, tm, &o0, &o1, &first); break;
                case 5: pt_slab_pk2<5>(rec, q, tm, &o0, &o1, &first); break;
                case 6: pt_slab_pk2<6>(rec, q, tm, &o0, &o1, &first); break;
                default: pt_slab_pk2<7>(rec, q, tm, &o0, &o1, &first); break;
            }
        }
        if (m0) v |= 2;
        if (o0) v |= 4;
        if ((m0 != 0) != (m1 != 0) || (o0 != 0) != (o1 != 0)) v |= 8;
        verdict[i] = v;
    }
    return PT_OK;
}

// What the last launch of the context left in its pixel lists (tests; the launch must have been closed - pt_render, or pt_render_finish): out[0] the records (0: that
// launch had no lists - PORTRAYER_PIXEL_LISTS=0, several pixels per wavefront, another mode or kernel), out[1] those that are background (empty, infinite tail), out[2]
// those cut at the cap (finite tail), out[3] those marked "take the walk", out[4 + n] those with n entries, n = 0 .. PT_PL_K (5 + PT_PL_K words in all). The records are copied back and counted here.
extern "C" int pt_test_pixel_list_summary(pt_context* c, uint64_t* out) {
    if (!c || !out) return PT_ERR_ARGUMENT;
    for (uint32_t k = 0; k < 5u + PT_PL_K; k++) out[k] = 0;
    const PtLaunchPlan& p = c->last.plan;
    if (!p.pixel_lists) return PT_OK;
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipDeviceSynchronize());
    std::vector<uint32_t> rec((size_t)p.n_slots * PT_PL_WORDS);
    const pt_context::Slot& sl = c->slot[c->last.slot];
    if (sl.eye_tab.bytes < p.queue_off) return pt_fail(c, PT_ERR_ARGUMENT, "the slot's buffer no longer holds that launch's lists");
    PT_HIP(c, hipMemcpy(rec.data(), (const char*)sl.eye_tab.p + p.records_off, rec.size() * 4, hipMemcpyDeviceToHost));
    out[0] = p.n_slots;
    for (uint32_t i = 0; i < p.n_slots; i++) {
        const uint32_t head = rec[(size_t)i * PT_PL_WORDS], tail = rec[(size_t)i * PT_PL_WORDS + 1];
        if (head & PT_PL_WALK) { out[3]++; continue; }
        const uint32_t n = head & 255u;
        if (n > PT_PL_K) return pt_fail(c, PT_ERR_TRAVERSAL, "a pixel list longer than its record");
        if (n == 0 && tail == PT_PL_INF_BITS) out[1]++;
        if (tail != PT_PL_INF_BITS) out[2]++;
        out[4 + n]++;
    }
    return PT_OK;
}

// Host-side run (no GPU involved) of the pixel lists' beam test (pt_pixel_list.h) beside the walk's own slab test: case i is a camera (cameras[19 i ..]: eye, rows 0..2 of
// view_to_world, fov_factor, aspect, width, height - PtCamera's fields in order), a pixel (pixels[2 i ..]: x, y), a sample of it (jitters[2 i ..] in [0, 1): the ray of
// pt_camera_ray(x + jx, y + jy)) and a box (3 floats each). Out per case: accept = pt_beam_box's verdict for the pixel's beam, bound = the bound it stores (0 where it
// rejects), walk = what the walk does with the box for that sample's ray and no bound on t (pt_raypk's constants): bit 0 pt_slab_pk2<PT_OCT_MIXED> accepts, bit 1 the form of
// the ray's own octant accepts (a ray with a switched-off axis has none: bit 1 repeats bit 0); rays (optional, 6 doubles per case): that ray's origin and direction.
// Tests check that walk != 0 never comes with accept == 0, and that bound never exceeds the exact entry parameter.
// (`stride` words per case in `rects`: x, y and, where stride is 4, nx, ny - otherwise the pixel's 1, 1)
static int pt_test_beam_cases(uint64_t n, const double* cameras, const uint32_t* rects, uint32_t stride, const double* jitters, const float* box_lo, const float* box_hi,
                              int32_t* accept, float* bound, int32_t* walk, double* rays) {
    if (!cameras || !rects || !jitters || !box_lo || !box_hi || !accept || !bound || !walk) return PT_ERR_ARGUMENT;
    for (uint64_t i = 0; i < n; i++) {
        PtCamera cam;
        const double* cp = cameras + 19 * i;
        for (int k = 0; k < 3; k++) cam.eye[k] = cp[k];
        for (int k = 0; k < 12; k++) cam.view_to_world[k] = cp[3 + k];
        cam.fov_factor = cp[15]; cam.aspect = cp[16]; cam.width = cp[17]; cam.height = cp[18];
        const uint32_t x = rects[stride * i], y = rects[stride * i + 1];
        const float* lo = box_lo + 3 * i;
        const float* hi = box_hi + 3 * i;
        const PtBeam beam = stride == 4u ? pt_beam_setup(cam, (double)x, (double)y, (double)rects[4 * i + 2], (double)rects[4 * i + 3]) : pt_beam_setup(cam, (double)x, (double)y);
        float b = 0.0f;
        accept[i] = pt_beam_box(beam, lo, hi, &b) ? 1 : 0;
        bound[i] = accept[i] ? b : 0.0f;
        const PtRay r = pt_camera_ray(cam, (double)x + jitters[2 * i], (double)y + jitters[2 * i + 1]);
        if (rays) { rays[6 * i] = r.o.x; rays[6 * i + 1] = r.o.y; rays[6 * i + 2] = r.o.z; rays[6 * i + 3] = r.d.x; rays[6 * i + 4] = r.d.y; rays[6 * i + 5] = r.d.z; }
        PtRayPk q;
        int s[3];
        s[0] = pt_raypk_axis(r.o.x, r.d.x, &q.a[0], &q.b[0]); s[1] = pt_raypk_axis(r.o.y, r.d.y, &q.a[1], &q.b[1]); s[2] = pt_raypk_axis(r.o.z, r.d.z, &q.a[2], &q.b[2]);
        pt_u32x16 rec;
        for (int k = 0; k < 16; k++) rec[k] = 0u;
        for (int k = 0; k < 3; k++) {
            uint32_t l, h;
            memcpy(&l, lo + k, 4); memcpy(&h, hi + k, 4);
            rec[2 * k] = rec[2 * k + 1] = l; rec[6 + 2 * k] = rec[6 + 2 * k + 1] = h;
        }
        unsigned long long m0 = 0, m1 = 0, first = 0, o0 = 0, o1 = 0;
        pt_slab_pk2<PT_OCT_MIXED>(rec, q, INFINITY, &m0, &m1, &first);
        o0 = m0; o1 = m1;
        if (s[0] && s[1] && s[2]) {
            switch ((s[0] == 2 ? 1 : 0) | (s[1] == 2 ? 2 : 0) | (s[2] == 2 ? 4 : 0)) {
                case 0: pt_slab_pk2<0>(rec, q, INFINITY, &o0, &o1, &first); break;
                case 1: pt_slab_pk2<1>(rec, q, INFINITY, &o0, &o1, &first); break;
                case 2: pt_slab_pk2<2>(rec, q, INFINITY, &o0, &o1, &first); break;
                case 3: pt_slab_pk2<3>(rec, q, INFINITY, &o0, &o1, &first); break;
                case 4: pt_slab_pk2<4>(rec, q, INFINITY, &o0, &o1, &first); break;
                case 5: pt_slab_pk2<5>(rec, q, INFINITY, &o0, &o1, &first); break;
                case 6: pt_slab_pk2<6>(rec, q, INFINITY, &o0, &o1, &first); break;
                default: pt_slab_pk2<7>(rec, q, INFINITY, &o0, &o1, &first); break;
            }
        }
        walk[i] = (m0 ? 1 : 0) | (o0 ? 2 : 0);
    }
    return PT_OK;
}
extern "C" int pt_test_pixel_beam(uint64_t n, const double* cameras, const uint32_t* pixels, const double* jitters, const float* box_lo, const float* box_hi,
                                  int32_t* accept, float* bound, int32_t* walk, double* rays) {
    return pt_test_beam_cases(n, cameras, pixels, 2u, jitters, box_lo, box_hi, accept, bound, walk, rays);
}
// pt_test_pixel_beam with a rectangle per case (rects[4 i ..]: x, y, nx, ny - the beam of the sample positions in [x, x + nx] x [y, y + ny], pt_pixel_list.h 7.; the list
// kernel's tile beam is nx = ny = 8) and the sample's position inside it (offsets[2 i ..] in [0, nx] x [0, ny]: the ray of pt_camera_ray(x + ox, y + oy)). nx = ny = 1 is
// pt_test_pixel_beam's case, bit for bit.
extern "C" int pt_test_rect_beam(uint64_t n, const double* cameras, const uint32_t* rects, const double* offsets, const float* box_lo, const float* box_hi,
                                 int32_t* accept, float* bound, int32_t* walk, double* rays) {
    return pt_test_beam_cases(n, cameras, rects, 4u, offsets, box_lo, box_hi, accept, bound, walk, rays);
}

// The last launch's pixel-list records as the list kernel wrote them (tests; the launch must have been closed, as for pt_test_pixel_list_summary): info[0] the records (0:
// that launch had no lists), info[1] the words of a record (PT_PL_WORDS), info[2] the entries a record holds at most (PT_PL_K), info[3] the scene's flattened nodes. Where
// `out` is not NULL and `words` >= info[0] info[1], the records are copied to it; with fewer words (0: a query of the sizes) nothing is copied.
extern "C" int pt_test_pixel_list_records(pt_context* c, uint32_t* out, uint64_t words, uint64_t* info) {
    if (!c || !info) return PT_ERR_ARGUMENT;
    const PtLaunchPlan& p = c->last.plan;
    info[0] = 0; info[1] = PT_PL_WORDS; info[2] = PT_PL_K; info[3] = p.n_nodes;
    if (!p.pixel_lists) return PT_OK;
    info[0] = p.n_slots;
    const size_t need = (size_t)p.n_slots * PT_PL_WORDS;
    if (!out || words < need) return PT_OK;
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipDeviceSynchronize());
    const pt_context::Slot& sl = c->slot[c->last.slot];
    if (sl.eye_tab.bytes < p.queue_off) return pt_fail(c, PT_ERR_ARGUMENT, "the slot's buffer no longer holds that launch's lists");
    PT_HIP(c, hipMemcpy(out, (const char*)sl.eye_tab.p + p.records_off, need * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}

// The last launch's queue of the pixels that need the render kernel (pt_pixel_list.h) as the list kernel left it (tests; the launch must have been closed): info[0] 1 where
// that launch had a queue, else 0; info[1] the count in header word 1; info[2] the launch's pixel slots (what the queue can hold). Where `out` is not NULL and `words` >=
// info[1], the first info[1] slot ids are copied to it.
extern "C" int pt_test_pixel_list_queue(pt_context* c, uint32_t* out, uint64_t words, uint64_t* info) {
    if (!c || !info) return PT_ERR_ARGUMENT;
    const PtLaunchPlan& p = c->last.plan;
    info[0] = info[1] = 0; info[2] = p.n_slots;
    if (!p.background_skip) return PT_OK;
    info[0] = 1;
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipDeviceSynchronize());
    const pt_context::Slot& sl = c->slot[c->last.slot];
    if (sl.eye_tab.bytes < p.queue_off + (size_t)p.n_slots * 4) return pt_fail(c, PT_ERR_ARGUMENT, "the slot's buffer no longer holds that launch's queue");
    uint32_t head[2] = {0u, 0u};
    PT_HIP(c, hipMemcpy(head, (const char*)sl.eye_tab.p + p.header_off, sizeof head, hipMemcpyDeviceToHost));
    if (!(head[0] & PT_PL_QUEUE)) return pt_fail(c, PT_ERR_TRAVERSAL, "the header of a launch with a queue does not say so");
    info[1] = head[1];
    if (head[1] > p.n_slots) return pt_fail(c, PT_ERR_TRAVERSAL, "more pixels queued than the launch has slots");
    if (!out || words < head[1] || head[1] == 0u) return PT_OK;
    PT_HIP(c, hipMemcpy(out, (const char*)sl.eye_tab.p + p.queue_off, (size_t)head[1] * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}

// Host-side run (no GPU involved) of pt_background_sum (pt_shade.h): the sum of `samples` samples of the colour rgb[0..2] under the summation contract -> out[0..2].
extern "C" int pt_test_background_sum(const double* rgb, uint32_t samples, double* out) {
    if (!rgb || !out || samples == 0u) return PT_ERR_ARGUMENT;
    PtRenderArgs a;
    memset(&a, 0, sizeof a);
    a.background = rgb; a.background_rows = 1; a.width = a.height = 1;
    a.samples = samples; a.n_chunks = (samples + PT_SAMPLE_CHUNK - 1u) / PT_SAMPLE_CHUNK;
    const PtVec3 s = pt_background_sum(a, 0u, 0u);
    out[0] = s.x; out[1] = s.y; out[2] = s.z;
    return PT_OK;
}

// Host-side run (no GPU involved) of the certain-shadow test (pt_certain.h): case i is a node of `type` with the records fwd[12 i ..], inv[12 i ..] (rows 0..2 of its two
// matrices), a shaded point P[3 i ..] and a light position L[3 i ..]. out_certain[i]: the table routine gave the node a ball and the lane test, on the floats the kernel would
// hold, says "certainly hit"; out_exact_hit[i]: the reference's own test of that node for the shadow ray {P, (L - P) / |L - P|} over [EPSILON, INF) (pt_ray_to_local,
// pt_unit_prim_hit). Tests check that certain never comes without exact_hit.
extern "C" int pt_test_certain_shadow(uint64_t n, int type, const double* fwd, const double* inv, const double* P, const double* L, int32_t* out_certain, int32_t* out_exact_hit) {
    if (!fwd || !inv || !P || !L || !out_certain || !out_exact_hit || type < 0 || type > 7) return PT_ERR_ARGUMENT;
    for (uint64_t i = 0; i < n; i++) {
        float ball[4];
        pt_certain_ball((uint32_t)type, fwd + 12 * i, inv + 12 * i, ball);
        const PtVec3 p = pt_v3(P[3 * i], P[3 * i + 1], P[3 * i + 2]), l = pt_v3(L[3 * i], L[3 * i + 1], L[3 * i + 2]);
        out_certain[i] = ball[3] > 0.0f && pt_certain_lane(ball, (float)p.x, (float)p.y, (float)p.z, (float)l.x, (float)l.y, (float)l.z) ? 1 : 0;
        PtRay r;
        r.o = p;
        const PtVec3 hit_to_light = l - p;
        r.d = hit_to_light / pt_length(hit_to_light);
        const PtRay local = pt_ray_to_local(inv + 12 * i, r);
        double t;
        uint32_t part = 0;
        out_exact_hit[i] = pt_unit_prim_hit((uint32_t)type, local, PT_EPSILON, INFINITY, &t, &part) ? 1 : 0;
    }
    return PT_OK;
}

// Host-side run (no GPU involved) of the dark-light test (pt_certain.h 4.-8.): case i is a node of `type` with the records fwd[12 i ..], inv[12 i ..], a shaded point P[3 i ..]
// and a light at L[3 i ..] with the area vectors area[6 i ..] (area_a, area_b; NULL: point lights). out_flagged[i]: the table routines gave the node a ball and found the light
// enclosed in it; out_guard[i]: the lane guard, on the floats the kernel would hold, lets P through (0 where not flagged); out_exact_hit[i]: the reference's own test of that
// node for the shadow ray {P, (L - P) / |L - P|} over [EPSILON, INF), as in pt_test_certain_shadow. Tests check that flagged and guard never come without exact_hit.
extern "C" int pt_test_dark_light(uint64_t n, int type, const double* fwd, const double* inv, const double* P, const double* L, const double* area, int32_t* out_flagged,
                                  int32_t* out_guard, int32_t* out_exact_hit) {
    if (!fwd || !inv || !P || !L || !out_flagged || !out_guard || !out_exact_hit || type < 0 || type > 7) return PT_ERR_ARGUMENT;
    for (uint64_t i = 0; i < n; i++) {
        float ball[4], rec[4];
        pt_certain_ball((uint32_t)type, fwd + 12 * i, inv + 12 * i, ball);
        double light[15];
        for (int k = 0; k < 15; k++) light[k] = 0.0;
        for (int k = 0; k < 3; k++) light[k] = L[3 * i + k];
        if (area) for (int k = 0; k < 6; k++) light[9 + k] = area[6 * i + k];
        const PtVec3 p = pt_v3(P[3 * i], P[3 * i + 1], P[3 * i + 2]), l = pt_v3(light[0], light[1], light[2]);
#ifndef PT_NO_DARK_LIGHTS
        out_flagged[i] = pt_dark_light(light, ball, rec) ? 1 : 0;
        out_guard[i] = out_flagged[i] && pt_dark_lane(rec, (float)p.x, (float)p.y, (float)p.z) ? 1 : 0;
#else
        (void)rec;
        out_flagged[i] = out_guard[i] = 0;
#endif
        PtRay r;
        r.o = p;
        const PtVec3 hit_to_light = l - p;
        r.d = hit_to_light / pt_length(hit_to_light);
        const PtRay local = pt_ray_to_local(inv + 12 * i, r);
        double t;
        uint32_t part = 0;
        out_exact_hit[i] = pt_unit_prim_hit((uint32_t)type, local, PT_EPSILON, INFINITY, &t, &part) ? 1 : 0;
    }
    return PT_OK;
}

// The dark-light records of the context's last launch (tests; the launch must have been closed): info[0] the lights that launch had records for (0: none - another mode,
// no occluder table, -DPT_NO_DARK_LIGHTS), info[1] the words of a record (PT_DARK_WORDS). Where `out` is not NULL and `words` >= info[0] info[1], the records are copied to it.
extern "C" int pt_test_dark_lights(pt_context* c, uint32_t* out, uint64_t words, uint64_t* info) {
    if (!c || !info) return PT_ERR_ARGUMENT;
    info[0] = 0; info[1] = PT_DARK_WORDS;
    const PtLaunchPlan& p = c->last.plan;
    if (p.dark_bytes == 0) return PT_OK;
    info[0] = p.n_lights;
    const size_t need = p.dark_bytes / 4;
    if (!out || words < need) return PT_OK;
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipDeviceSynchronize());
    const pt_context::Slot& sl = c->slot[c->last.slot];
    if (sl.misc.bytes < p.occ_off) return pt_fail(c, PT_ERR_ARGUMENT, "the slot's buffer no longer holds that launch's records");
    PT_HIP(c, hipMemcpy(out, (const char*)sl.misc.p + p.dark_off, p.dark_bytes, hipMemcpyDeviceToHost));
    return PT_OK;
}

// How a launch's traversal stacks are split between LDS and HBM - one place for the render kernels and every pass beside them, whose
// kernels lay their LDS out with the same code (pt_trace_wave: pt_wave_rows, pt_kd_layout).
// pt_stack_lds_cap: entries per lane kept in LDS = what `block_budget` bytes of LDS per block leave beside `frame_bytes` of other per-block data (1 KB a row), at most the
// scene's whole stack. The k-d walk keeps no saved bounds in HBM (round 5): its wavefront rows must hold the stack and, where the stack's slack is too small for it, the two
// rows of the path table (pt_kd_layout, PtKdSav) - also under PORTRAYER_LDS_STACK=1 (experiments / tests of the overflow path), which then only shrinks the LANES' stacks.
static bool pt_kd_semantics(int mode) { return mode == PT_MODE_KD || mode == PT_MODE_KD_NOMESH || mode == PT_MODE_KD_MESH; }
static int pt_stack_lds_cap(int mode, int stack_cap, size_t block_budget, size_t frame_bytes) {
    int lds_cap = block_budget > frame_bytes ? (int)((block_budget - frame_bytes) / (PT_BLOCK * 4)) : 0;
    lds_cap = pt_env_clamped("PORTRAYER_LDS_STACK", std::max(lds_cap, 2), 1, INT_MAX);
    int cap = std::min(lds_cap, stack_cap);
    if (pt_kd_semantics(mode)) cap = std::max(cap, (stack_cap + 63) / 64 + 2);
    return cap;
}
static int pt_stack_lds_cap(const PtSceneView& sc, size_t block_budget, size_t frame_bytes) { return pt_stack_lds_cap(sc.mode, sc.stack_cap, block_budget, frame_bytes); }
// pt_stack_column: entries of a lane's HBM stack column (PtStackSpill::gbase). + wave_rows: the wavefront's own stack takes LDS rows from the lanes' stacks (pt_wave_rows,
// pt_render_simple.h): eight, or what a deep tree needs; and at least everything a lane's own stack can reach (pt_trace_wave gives the lanes fewer LDS rows in the k-d semantics).
static size_t pt_stack_column(int stack_cap, int stack_lds_cap) {
    const int wave_rows = std::min(std::max(8, (stack_cap + 63) / 64), std::max(stack_lds_cap, 8));  // (pt_wave_rows: at most this many)
    const int stack_spill_entries = std::max(stack_cap - stack_lds_cap + wave_rows, 0);
    return (size_t)std::max(stack_spill_entries, stack_cap);
}
static size_t pt_stack_column(const PtSceneView& sc, int stack_lds_cap) { return pt_stack_column(sc.stack_cap, stack_lds_cap); }

// What a pass's sizing dispatch reads of the host-side fields. The passes that only walk (primary visibility, ray queries): the LDS stack area is sized like a
// render's for the waves per SIMD the mode's instantiation is compiled for, with no hit frame beside the stacks.
static void pt_walk_sizing(PtRenderArgs& r, int waves) {
    r.stack_lds_cap = pt_stack_lds_cap(r.scene, pt_block_budget(waves), 0);
    r.grid_share = 1;
}
// The interpreter passes (radiance, the film's): LDS per block as a render's interpreter kernel has it - three blocks per CU, the stack area beside the hit
// frame and, in scenes whose hits spawn rays, the youngest parked frame of every lane. Returns which <TEX, PARK> instantiation runs.
struct PtInterp { bool tex, park; };
static PtInterp pt_interp_sizing(const pt_context* c, PtRenderArgs& r) {
    PtInterp k;
    k.tex = r.scene.mat_maps != nullptr;
    k.park = pt_spawns(c->traits) && pt_env_park();  // (as for a render)
    r.park_slots = k.park ? 1 : 0;
    const size_t frame_bytes = (size_t)(PT_LDS_FRAME_F64 + r.park_slots * PT_PARK_F64) * PT_BLOCK * 8;
    r.stack_lds_cap = pt_stack_lds_cap(r.scene, pt_block_budget(3), frame_bytes);  // (pt_radiance_waves, pt_film_waves)
    r.grid_share = 1;
    return k;
}

// ------------------------------------------------------------------------------------------------
// Which render kernel a scene runs: PtRenderArgs::run_variant, the waves per SIMD its instantiation is compiled for (PtRenderArgs::four_waves: 0 = three),
// the parked frames kept in LDS and the LDS a block may take. One rule per kernel family - pt_choose_kernel picks the family, the family's function its
// wave count - from what the scene says (PtSceneTraits), its mode, whether it is textured, and the PORTRAYER_WAVES, KD_WAVES, CHAIN, CHAIN_WAVES, PARK, FORK and
// LDS_BUDGET_KB switches, which nothing else reads for this. No context, no HIP call (pt_test_kernel_choice).
// ------------------------------------------------------------------------------------------------
// The straight-line kernel, flat_scene / hierarchical semantics.
// The 4-waves-per-SIMD kernel for scenes where the tree walk outweighs the shading: many scene-level nodes or many instanced
// triangles, nothing reflective, flat_scene semantics (measured: big-scene +8.7 %, big-soup +6.8 %; macho-cows
// with its 23 nodes and 17,500 triangles -8 %; reflective scenes and the k-d walk lose, profiles/r02/notes.md)
static int pt_line_waves(const PtSceneTraits& t, int mode, bool tex) {
    if (const int wv = pt_env_clamped("PORTRAYER_WAVES", -1, 0, 6); wv >= 0) {
        if (wv < 4) return 0;
        if (wv >= 5 && (mode == PT_MODE_FLAT_NOMESH || mode == PT_MODE_HIER_NOMESH)) return PT_LINE_TOP_WAVES;
        return (wv >= 5 && (mode == PT_MODE_FLAT || mode == PT_MODE_HIER_MESH)) ? PT_MESH_TOP_WAVES : 4;
    }
    const bool hier = t.traverse == PT_TRAVERSE_HIER, many_tris = t.instanced_tris >= 65536;
    // hierarchical semantics (round 3, straight-line kernel): mesh-free scenes with many nodes gain like flat_scene ones (big-scene 25.7 ->
    // 29.4 Gray/s at 4 waves); with mesh instances the walk carries a second ray and spills at 128 registers (macho-cows 16.4 -> 12.0) unless
    // the triangle trees dominate (the 1.25 M-triangle soup: equal)
    // Since the register work of round 3 (arguments re-read, colour parked in LDS, an instantiation of the hierarchical semantics without
    // the KDMesh walker) scenes with plain Mesh instances of any size gain too (c41: macho-cows 21.4 -> 23.4 Gray/s, hierarchical 18.7 -> 19.7);
    // with KDMesh trees the kernels still spill 100+ registers at 128 and stay at 3 waves unless the triangle trees dominate.
    const bool plain_meshes = t.has_meshes && !t.has_kdmesh;
    // traversal-heavy scene: a kernel compiled for more than 3 waves per SIMD
    const bool heavy = hier ? ((!t.has_meshes && t.n_nodes >= 256) || many_tris) : (t.n_nodes >= 256 || many_tris);
    // ... or, while the scene has no texture maps: any scene with plain Mesh instances (textured: flat_scene loses 10 % at 4 waves, c45)
    // The hierarchical semantics without KDMesh trees gain at 4 waves whatever the scene (their leaf tests wait for a path record and a matrix per
    // level): macho-cows +5 %, fish (textured) +5 %, normal-mapping (11 textured primitives) +12 %, the mirror scene's chain kernel +9 % (c41, c45).
    if (!(heavy || (plain_meshes && !tex) || (hier && !t.has_kdmesh))) return 0;
    // mesh-free scenes go one further: 5 waves per SIMD (96 registers, 17 of the kernel's spilled; big-scene 34.4 -> 37.0, hierarchical
    // 29.4 -> 32.5 Gray/s; the k-d walk, 50 spilled, loses and stays at 4)
    if (heavy && !t.has_meshes) return PT_LINE_TOP_WAVES;
    // ... and so do scenes of very many triangles in plain Mesh instances (round 4, c29: their walks wait for node fetches - 3 -> 4 waves was +18 % -; the 1.25 M-triangle
    // scenes +3.7 % / +3.2 %, hierarchical +2.6 %, at 96 registers with 57 spilled; macho-cows, 17,500 triangles, loses 15 % and stays at 4)
    // Round 5 (c47 / c48, after the tree step and the instance walk issue fewer scalar instructions): flat_scene is now FASTER at 4 waves (big-soup 18.96 -> 18.75 ms,
    // big-mesh 19.16 -> 18.86; 18 spilled registers instead of 69) and takes 4; the hierarchical semantics still gain 1 % at 5 and keep them.
    return (plain_meshes && many_tris && hier && !tex) ? PT_MESH_TOP_WAVES : 4;
}

// The straight-line kernel, k-d semantics.
// The k-d semantics: mesh-free scenes with many nodes take the 4-wave straight-line kernel too (big-scene 35.7 -> 30.7 ms: the per-lane
// k-d walk waits on its own loads, a fourth wavefront per SIMD hides more of that than the 4 spilled registers cost); with mesh
// instances the walk needs the registers (167 at 3 waves). PORTRAYER_KD_WAVES=3|4 overrides.
// Round 4 (one walk per wavefront, pt_trace_packet_kd): mesh-free scenes with many nodes at 5 waves (big-scene 29.2 -> 28.1 ms, c10), scenes with plain
// Mesh instances (PT_MODE_KD_MESH: no KDMesh walker compiled in) at 4; with KDMesh trees the kernel needs its 168 registers.
static int pt_line_waves_kd(const PtSceneTraits& t, int mode) {
    if (const int wv = pt_env_clamped("PORTRAYER_KD_WAVES", -1, 0, 6); wv >= 0) {
        return (wv < 4 || mode == PT_MODE_KD) ? 0 : ((wv >= 5 && mode == PT_MODE_KD_NOMESH) ? 5 : 4);
    }
    return (mode == PT_MODE_KD_NOMESH && t.n_nodes >= 256) ? 5 : (mode == PT_MODE_KD_MESH ? 4 : 0);
}

// The chain kernel.
// 4 waves per SIMD in the flat_scene semantics (mirror scene 25.5 -> 26.8 Gray/s, c34: ten bounces per sample leave a lot of latency to hide),
// 3 in the hierarchical ones (182 spilled registers at 128: 19.3 -> 14.8) and the k-d ones. PORTRAYER_CHAIN_WAVES=3|4 overrides.
// (Only where that was measured or the compiler's figures are like the measured case's: untextured, no KDMesh trees - those
// instantiations spill 57 / 142 registers at 128.)
static int pt_chain_waves(int mode, bool tex) {
    if (const int wv = pt_env_clamped("PORTRAYER_CHAIN_WAVES", -1, 0, 6); wv >= 0) return (wv == 4 && mode != PT_MODE_KD) ? 4 : 0;
    const bool flat_sem = (mode == PT_MODE_FLAT || mode == PT_MODE_FLAT_NOMESH || mode == PT_MODE_HIER_MESH) && !tex;  // (HIER_MESH: 22.2 -> 24.2, c41)
    return (flat_sem || (mode == PT_MODE_KD_MESH && !tex)) ? 4 : 0;
}

static PtKernelChoice pt_choose_kernel(const PtSceneTraits& t, int mode, bool tex) {
    PtKernelChoice k;
    k.needs_spill = pt_needs_spill(t);
    // Scenes whose hits spawn rays need the interpreter kernel (3 waves per SIMD); the others run the straight-line kernel at 3 or
    // 4 waves per SIMD.
    if (!pt_spawns(t)) {
        k.four_waves = pt_kd_semantics(mode) ? pt_line_waves_kd(t, mode) : pt_line_waves(t, mode, tex);
        k.run_variant = k.four_waves >= 5 ? PT_RUN_LINE5 : (k.four_waves ? PT_RUN_LINE4 : PT_RUN_LINE3);  // (LINE5: the densest instantiation the mode has)
    } else {
        // parked recursion frames kept in LDS (pt_shade.h): only scenes that park frames at all have any
        const bool park = pt_env_park();
        // every reflective material is opaque (no index of refraction): a hit spawns at most one ray, the recursion is a chain
        const bool chain = t.reflective_opaque != 0 && pt_env_on("PORTRAYER_CHAIN", true);  // 0: the interpreter kernel also for scenes whose recursion is a chain (A/B runs, tests)
        if (chain && park) {
            k.run_variant = PT_RUN_CHAIN;
            k.park_slots = 0;  // no frame in LDS: the parked colours go straight to the lane's HBM lines
            k.four_waves = pt_chain_waves(mode, tex);
        } else {
            // Fork / join of refracted subtrees (pt_shade.h) is built, parity-green and OFF by default: it fills the idle lanes and still loses
            // (transmission-refraction 11.4 -> 8.6 Gray/s, profiles/r03/notes.md section 4): the subtrees other lanes walk are other rays, and the
            // one walk per wavefront pays for the union of their paths. PORTRAYER_FORK=1 switches it on for scenes that qualify.
            // fork / join of refracted subtrees (pt_shade.h) needs a recursion that draws no random numbers and a dielectric material to be of use:
            // no hit draws random numbers after the jitter (no area light, no glossy material): refracted subtrees may be walked by other lanes
            const bool forkable = !t.reflective_opaque && !t.glossy && !t.area_light && t.n_lights <= PT_LIGHT_ROUND;
            const bool fork = forkable && park && pt_env_on("PORTRAYER_FORK", false);
            k.run_variant = park ? (fork ? PT_RUN_INTERP_FORK : PT_RUN_INTERP_PARK) : PT_RUN_INTERP;
            k.park_slots = park ? 1 : 0;
        }
    }
    k.block_budget = pt_block_budget(k.four_waves ? k.four_waves : 3);
    if (const int kb = pt_env_clamped("PORTRAYER_LDS_BUDGET_KB", 0, 16, 160)) k.block_budget = (size_t)kb * 1024;  // experiment: 80 = two blocks per CU
    return k;
}

// pt_stats.kernel_variant of a choice (without PT_KERNEL_COUNTING, the launch's own)
static uint32_t pt_choice_variant(const PtKernelChoice& k, bool tex) {
    const int v = k.run_variant;
    const bool line = v == PT_RUN_LINE3 || v == PT_RUN_LINE4 || v == PT_RUN_LINE5;
    return (k.four_waves ? (uint32_t)k.four_waves : 3u) | ((line || v == PT_RUN_CHAIN) ? 0u : PT_KERNEL_INTERPRETER) | (v == PT_RUN_CHAIN ? PT_KERNEL_CHAIN : 0u) |
           ((v == PT_RUN_INTERP_PARK || v == PT_RUN_INTERP_FORK) ? PT_KERNEL_PARK : 0u) | (v == PT_RUN_INTERP_FORK ? PT_KERNEL_FORK : 0u) | (tex ? PT_KERNEL_TEXTURED : 0u);
}

extern "C" int pt_test_kernel_choice(const pt_scene_traits* traits, int mode, int textured, uint32_t* kernel_mode, uint32_t* kernel_variant) {
    if (!traits || !kernel_mode || !kernel_variant) return PT_ERR_ARGUMENT;
    if (mode < 0) mode = pt_scene_mode(*traits);
    *kernel_mode = (uint32_t)mode;
    *kernel_variant = pt_choice_variant(pt_choose_kernel(*traits, mode, textured != 0), textured != 0);
    return PT_OK;
}

// ------------------------------------------------------------------------------------------------
// A render launch, planned (PtLaunchPlan, pt_context.h): how the work is dealt, the bytes of the slot's five buffers, where each table and list lies in
// `misc` and `eye_tab`, and which of them this launch has - from the scene's traits, the launch's shape (pt_launch_query, the fields of PtRenderArgs a launch depends
// on), the resident grid and the PORTRAYER_* switches. No context, no HIP call (pt_test_launch_plan). Two steps, because the size query needs the kernel and the
// plan needs the grid: pt_plan_kernel, pt_dispatch(launch = false), pt_plan_launch; pt_render_common commits the result.
// ------------------------------------------------------------------------------------------------
// What the build compiled in (EXTRA_HIPFLAGS / make variant; the Makefile's SWITCHES), asked here and nowhere else in the host code. (A macro that is not defined
// stringifies to its own name.)
#define PT_STRINGIFY_(x) #x
#define PT_STRINGIFY(x) PT_STRINGIFY_(x)
constexpr bool pt_same_text(const char* a, const char* b) { return *a == *b && (*a == 0 || pt_same_text(a + 1, b + 1)); }
#define PT_BUILT_WITH(flag) (!pt_same_text(#flag, PT_STRINGIFY(flag)))
constexpr bool PT_EYE_TABLE = !PT_BUILT_WITH(PT_NO_EYE_TABLE), PT_CERTAIN_SHADOW = !PT_BUILT_WITH(PT_NO_CERTAIN_SHADOW), PT_DARK_LIGHTS = !PT_BUILT_WITH(PT_NO_DARK_LIGHTS),
               PT_PIXEL_LISTS = !PT_BUILT_WITH(PT_NO_PIXEL_LISTS), PT_BACKGROUND_SKIP = !PT_BUILT_WITH(PT_NO_BACKGROUND_SKIP),
               PT_LIST_STATS = PT_BUILT_WITH(PT_PIXEL_LIST_STATS),  // the counting build evaluates the lists beside its walk (pt_render_simple.h): it gets them too
               PT_DEPTH_FIRST = PT_BUILT_WITH(PT_PL_DEPTH_FIRST);   // the list kernel as it was before round 13: it fills no queue

typedef pt_launch_query PtLaunchQuery;
static bool pt_parse_decimal(const char* text, unsigned long long* v) {
    char* end = nullptr;
    *v = strtoull(text, &end, 10);
    return end != text && !*end;
}

// Step 1: the kernel, its variant word and the LDS split of its traversal stacks - what the size query (pt_dispatch) reads.
// LDS per block = traversal stack (as much of it as leaves room for the kernel's blocks per CU) + the shaded hit's frame (+ a parked one); deeper stack entries live in
// HBM (PtStackSpill).
static void pt_plan_kernel(const PtLaunchQuery& q, PtLaunchPlan* plan) {
    PtLaunchPlan& p = *plan;
    p.choice = pt_choose_kernel(q.traits, q.mode, q.textured != 0);
    p.kernel_mode = (uint32_t)q.mode;
    p.kernel_variant = pt_choice_variant(p.choice, q.textured != 0) | (q.stats ? PT_KERNEL_COUNTING : 0u);
    const size_t frame_bytes = (size_t)(PT_LDS_FRAME_F64 + p.choice.park_slots * PT_PARK_F64) * PT_BLOCK * 8;
    p.stack_lds_cap = pt_stack_lds_cap(q.mode, q.stack_cap, p.choice.block_budget, frame_bytes);
    p.grid_share = 1;  // (a share of the resident blocks per launch was tried for ranks that share a GPU, round 5 c23: their kernels do not run side by side - 35.5 -> 14.3 Gray/s)
}

// Step 2, with q.grid = the resident blocks pt_dispatch answered. PT_ERR_ARGUMENT and *why for a malformed PORTRAYER_OCC_SEED, PIXEL_LIST_CAP or PIXEL_LIST_PENDING.
static int pt_plan_launch(const PtLaunchQuery& q, PtLaunchPlan* plan, std::string* why) {
    PtLaunchPlan& p = *plan;
    const bool flat_nomesh = q.mode == PT_MODE_FLAT_NOMESH, stats = q.stats != 0;
    p.n_slots = q.n_slots; p.n_nodes = q.n_nodes; p.n_lights = q.n_lights;

    // How the work items are handed out (pt_render_kernel): batches of consecutive items from one counter, or - scenes whose
    // hits can spawn rays, where an item in the glass costs hundreds of times its neighbour - one item at a time from
    // interleaved queues. transmission-refraction: wavefronts resident 47 % of the launch and 5.2 Gray/s with batches, 11+ without.
    const uint64_t resident_waves = (uint64_t)q.grid * (PT_BLOCK / 64);
    p.n_lanes = q.grid * PT_BLOCK;
    p.work_div = std::max<uint32_t>((uint32_t)resident_waves * 8u, 1u);  // batch = remaining items / (8 x resident wavefronts)
    p.batch_max = (uint32_t)pt_env_clamped("PORTRAYER_BATCH_MAX", PT_WORK_BATCH_MAX, 1, INT_MAX);
    // The queues also win wherever a wavefront gets few items (a small frame, one GPU's share of a frame: big-scene's 1/8 share +8 %,
    // macho-cows +13 %) and on the mesh-heavy scenes (+3-7 %); very long launches (> 2048 items per resident wavefront: 3840x2160x256)
    // are 1 % better off with batches.
    // (round 3's per-lane k-d walk was 1 % better off with batches; the wave-uniform one is not: big-scene +1.1 %, macho-cows +3.2 % with the queues, round 4 c68)
    const bool long_launch = (uint64_t)q.n_items > 2048ull * std::max<uint64_t>(resident_waves, 1);
    p.fine_queues = (uint32_t)pt_env_clamped("PORTRAYER_FINE_QUEUES", (pt_spawns(q.traits) || !long_launch) ? 16 : 0, 0, PT_FINE_QUEUES);  // 8 .. 32 queues measured alike, 64 and 4 about 1 % behind
    p.item_stride = 1;
    if (const char* e = getenv("PORTRAYER_ITEM_STRIDE")) {  // experiment (batches only): position q -> item (q * stride) mod n; "golden" = 0.618 n
        uint64_t st = strcmp(e, "golden") == 0 ? (uint64_t)((double)q.n_items * 0.6180339887498949) : (uint64_t)atoll(e);
        auto gcd = [](uint64_t x, uint64_t y) { while (y) { uint64_t t = x % y; x = y; y = t; } return x; };
        if (q.n_items > 2 && st != 1) { st = st % q.n_items; if (st < 1) st = 1; while (gcd(st, q.n_items) != 1) st++; p.item_stride = (uint32_t)st; }
    }

    p.spill = p.choice.needs_spill ? (size_t)p.n_lanes * PT_SPILL_DEPTHS * PT_SPILL_STRIDE * sizeof(double) : 16;
    p.stack_spill = (size_t)p.n_lanes * pt_stack_column(q.stack_cap, p.stack_lds_cap) * 4;  // (the k-d walk's saved bounds needed columns behind this until round 5)
    p.accum = (size_t)q.n_slots * q.n_chunks * 3 * sizeof(double);

    // `misc`. The occluder table of the mesh-free walks' shadow rays (pt_trace_packet): one word per (own 8x8 tile, light), behind the work queues, zeroed with them
    // before every launch - what it remembers comes from the frame being rendered, never from an earlier one. PORTRAYER_SHADOW_CACHE=0 leaves it out (A/B runs); so does
    // a table of more than 4 MB (many lights: zeroing it would cost more).
    p.occ_bytes = (size_t)(q.n_slots / 64) * q.n_lights * 4;
    if (!(flat_nomesh || q.mode == PT_MODE_HIER_NOMESH) || p.occ_bytes > ((size_t)4 << 20) || !pt_env_on("PORTRAYER_SHADOW_CACHE", true)) p.occ_bytes = 0;
    p.occ_row = std::max<uint32_t>(q.tiles_x / std::max<uint32_t>(q.tile_ranks, 1u), 1u);
    // PORTRAYER_OCC_SEED=all:K | <seed> (tests only): the table starts with hints the test chose (pt_occ_seed_kernel), not with zeros
    if (const char* e = getenv("PORTRAYER_OCC_SEED"); e && *e && p.occ_bytes) {
        unsigned long long v = 0;
        if (strncmp(e, "all:", 4) == 0) {
            if (!pt_parse_decimal(e + 4, &v) || v >= q.n_nodes) { *why = std::string("PORTRAYER_OCC_SEED=") + e + ": K must be a node index below " + std::to_string(q.n_nodes); return PT_ERR_ARGUMENT; }
            p.occ_seed = PT_OCC_SEED_ALL; p.occ_all = (uint32_t)v;
        } else {
            if (!pt_parse_decimal(e, &v)) { *why = std::string("PORTRAYER_OCC_SEED=") + e + ": expected all:<node> or a decimal seed"; return PT_ERR_ARGUMENT; }
            p.occ_seed = PT_OCC_SEED_HASHED; p.occ_seed_value = v;
        }
    }
    // The dark-light records (pt_dark_light_kernel; pt_certain.h 4.-8.) lie between the work queues and the occluder table, PT_DARK_WORDS words per light, zeroed with both:
    // the flat_scene launches that have an occluder table, so that the kernel finds them from PtRenderArgs::occluders alone. -DPT_NO_DARK_LIGHTS: no records.
    p.dark_bytes = (PT_DARK_LIGHTS && flat_nomesh && p.occ_bytes != 0) ? (size_t)q.n_lights * PT_DARK_WORDS * 4 : 0;
    p.dark_off = 256 + sizeof(PtCounters) + PT_FINE_QUEUES * PT_QUEUE_STRIDE * 4;
    p.occ_off = p.dark_off + p.dark_bytes;
    p.misc = p.occ_off + p.occ_bytes;

    // `eye_tab`. The eye table of the mesh-free flat_scene semantics (pt_render_simple.h: EYE_TABLE): every launch in that mode gets one, whichever kernel runs - the
    // counting, chain and interpreter kernels do not read it, and a launch's choice of kernel must never leave a kernel that does without.
    p.eye_table = PT_EYE_TABLE && flat_nomesh && q.n_nodes > 0;
    // The certain-shadow table (pt_render_simple.h: CERTAIN) behind it: the flat_scene launches that have an occluder table, whichever kernel runs.
    p.certain_table = PT_CERTAIN_SHADOW && flat_nomesh && q.n_nodes > 0 && p.occ_bytes != 0;
    // The kernel that fills the dark-light records reads the certain-shadow table. PORTRAYER_DARK_LIGHTS=0 (tests, A/B runs from one library): the records stay zero - no
    // light is skipped.
    p.dark_lights = p.certain_table && p.dark_bytes != 0 && pt_env_on("PORTRAYER_DARK_LIGHTS", true);
    // The per-pixel candidate lists (pt_pixel_list.h; pt_render_simple.h: PIXEL_LISTS) behind both: the launches whose kernel reads them - the plain straight-line kernels of
    // this mode where a wavefront is one pixel - and scenes whose node indices fit an entry's 16 bits. Their 64-byte header is written in every launch that has an eye table
    // (0: no lists). PORTRAYER_PIXEL_LISTS=0: none (the walk's image from the same library); PORTRAYER_PIXEL_LIST_CAP=k (tests only): a list holds k entries at most, so that
    // small scenes reach the tail bound and the fall-back; PORTRAYER_PIXEL_LIST_PENDING=n (tests only): the list kernel's pending list holds n nodes at most, so that tiles get
    // marked "take the walk". -DPT_NO_PIXEL_LISTS: no header, no lists, the kernels as they were (A/B).
    const int v = p.choice.run_variant;
    p.list_header = PT_PIXEL_LISTS && p.eye_table;
    p.pixel_lists = p.list_header && (PT_LIST_STATS || !stats) && (v == PT_RUN_LINE3 || v == PT_RUN_LINE4 || v == PT_RUN_LINE5) && q.k_log2 + q.c_log2 == 6u &&
                    q.n_nodes <= PT_PL_MAX_NODES && q.n_slots != 0 && pt_env_on("PORTRAYER_PIXEL_LISTS", true);
    p.list_cap = PT_PIXEL_LISTS ? PT_PL_K : 0u;
    p.list_pending = PT_PIXEL_LISTS ? 1024u : 0u;  // (the kernel's PT_PL_PENDING; the depth-first variant has its own stack and ignores it)
    if (PT_PIXEL_LISTS && !(pt_env_strict("PORTRAYER_PIXEL_LIST_CAP", 0, PT_PL_K, &p.list_cap, why) && pt_env_strict("PORTRAYER_PIXEL_LIST_PENDING", 1, p.list_pending, &p.list_pending, why)))
        return PT_ERR_ARGUMENT;
    // The queue of the pixels that need the render kernel (pt_pixel_list.h), behind the records: every launch that has lists. The render kernel deals only what is queued,
    // the finish kernel finishes the rest from the background. PORTRAYER_BACKGROUND_SKIP=0 (tests, A/B runs from one library): the lists as before, no queue, every
    // item dealt. -DPT_NO_BACKGROUND_SKIP: the kernels as they were, and the header's words say whether lists follow.
    p.background_skip = PT_BACKGROUND_SKIP && !PT_DEPTH_FIRST && !PT_LIST_STATS && p.pixel_lists && pt_env_on("PORTRAYER_BACKGROUND_SKIP", true);
    if (p.background_skip) p.item_stride = 1;  // (PORTRAYER_ITEM_STRIDE, an experiment: its stride is coprime to n_items, not to the queue's length)
    p.header_fill = (!PT_BACKGROUND_SKIP && p.pixel_lists) ? 1u : 0u;  // (all zero: the list kernel writes word 0 - what follows the header - and counts the queue in word 1)
    const uint32_t listed = p.pixel_lists ? q.n_slots : 0u;
    p.certain_off = (size_t)q.n_nodes * 12 * sizeof(double);
    p.header_off = p.list_header ? pt_pl_header_offset(q.n_nodes) : p.certain_off + (size_t)q.n_nodes * 4 * sizeof(float);
    p.records_off = p.header_off + (p.list_header ? 64u : 0u);
    p.queue_off = p.list_header ? p.header_off + pt_pl_bytes(listed, false) : p.records_off;
    p.eye_tab = !(p.eye_table || p.certain_table) ? 0 : (p.list_header ? p.header_off + pt_pl_bytes(listed, p.background_skip) : p.header_off);
    return PT_OK;
}

extern "C" int pt_test_launch_plan(const pt_launch_query* query, uint64_t* words, char* why, uint64_t why_bytes) {
    if (!query || !words) return PT_ERR_ARGUMENT;
    PtLaunchQuery q = *query;
    if (q.mode < 0) q.mode = pt_scene_mode(q.traits);
    PtLaunchPlan p;
    std::string err;
    pt_plan_kernel(q, &p);
    const int rc = pt_plan_launch(q, &p, &err);
    if (why && why_bytes) snprintf(why, (size_t)why_bytes, "%s", err.c_str());
    if (rc) return rc;
    const uint64_t w[PT_PLAN_WORDS] = {
        p.kernel_mode, p.kernel_variant, (uint64_t)p.choice.run_variant, (uint64_t)p.choice.four_waves, (uint64_t)p.choice.park_slots, p.choice.block_budget, p.choice.needs_spill,
        (uint64_t)p.stack_lds_cap, p.grid_share, p.n_lanes, p.work_div, p.batch_max, p.fine_queues, p.item_stride, p.spill, p.stack_spill, p.misc, p.accum, p.eye_tab,
        p.dark_off, p.dark_bytes, p.occ_off, p.occ_bytes, p.certain_off, p.header_off, p.records_off, p.queue_off,
        (p.occ_bytes ? PT_PLAN_HAS_OCCLUDERS : 0u) | (p.eye_table ? PT_PLAN_HAS_EYE_TABLE : 0u) | (p.certain_table ? PT_PLAN_HAS_CERTAIN_TABLE : 0u) |
            (p.dark_bytes ? PT_PLAN_HAS_DARK_RECORDS : 0u) | (p.dark_lights ? PT_PLAN_HAS_DARK_LIGHTS : 0u) | (p.list_header ? PT_PLAN_HAS_LIST_HEADER : 0u) |
            (p.pixel_lists ? PT_PLAN_HAS_PIXEL_LISTS : 0u) | (p.background_skip ? PT_PLAN_HAS_QUEUE : 0u),
        p.list_cap, p.list_pending, p.occ_row, (uint64_t)p.occ_seed, p.occ_seed == PT_OCC_SEED_ALL ? p.occ_all : p.occ_seed_value, p.header_fill};
    memcpy(words, w, sizeof w);
    return PT_OK;
}

// The fields of a launch's arguments that its plan depends on. PORTRAYER_NO_TEX: an experiment - the untextured kernel on a textured scene (wrong picture, timing only).
static PtLaunchQuery pt_launch_query_of(const PtSceneTraits& traits, PtRenderArgs& a, bool stats) {
    if (pt_env_set("PORTRAYER_NO_TEX")) a.scene.mat_maps = nullptr;
    PtLaunchQuery q = {};
    q.traits = traits; q.mode = a.scene.mode; q.textured = a.scene.mat_maps != nullptr; q.stats = stats;
    q.n_nodes = a.scene.n_nodes; q.n_lights = a.scene.n_lights; q.stack_cap = a.scene.stack_cap;
    q.n_slots = a.n_slots; q.n_items = a.n_items; q.n_chunks = a.n_chunks; q.k_log2 = a.k_log2; q.c_log2 = a.c_log2;
    q.tiles_x = a.div_tiles_x.d; q.tile_ranks = a.tile_ranks;
    return q;
}

static void pt_report_occ_seed(uint32_t n_occ) {
    if (pt_env_set("PORTRAYER_VERBOSE")) fprintf(stderr, "[pt_render] occluder table: %u entries seeded (PORTRAYER_OCC_SEED=%s)\n", n_occ, getenv("PORTRAYER_OCC_SEED"));
}

// Commits a planned launch to slot `slot_index` (< 0: the host-buffer path, pt_render, one frame at a time) on `stream`: the slot's buffers reserved, `a` pointed into
// them at the plan's offsets, `misc` zeroed, [the occluder table seeded,] ev0, the launch's tables and lists, the render kernel, the finish kernel, ev1, the copy of the
// flag and the counters. What the launch has and where it lies is the plan's to say, never this function's.
static int pt_render_common(pt_context* c, PtRenderArgs& a, bool stats, hipStream_t stream, int slot_index = -1) {
    if (slot_index < 0) {
        if (c->slot[c->slot_oldest].pending) return pt_fail(c, PT_ERR_ARGUMENT, "a render is in flight: pt_render_finish first");
        slot_index = c->slot_next;
    }
    PtLaunchQuery q = pt_launch_query_of(c->traits, a, stats);
    PtLaunchPlan plan;
    pt_plan_kernel(q, &plan);
    a.run_variant = plan.choice.run_variant; a.four_waves = plan.choice.four_waves; a.park_slots = plan.choice.park_slots;
    a.stack_lds_cap = plan.stack_lds_cap;
    a.grid_share = plan.grid_share;
    PT_HIP(c, pt_dispatch(a, stats, c->n_cu, stream, &q.grid, false));
    std::string why;
    if (int rc = pt_plan_launch(q, &plan, &why)) return pt_fail(c, rc, why);
    if (c->launch_seq == 0) c->launch_seq = (uint32_t)std::chrono::steady_clock::now().time_since_epoch().count() * 2654435761u;  // a different starting point in every context
    a.launch_nonce = ++c->launch_seq;
    a.n_lanes = plan.n_lanes; a.work_div = plan.work_div; a.batch_max = plan.batch_max; a.fine_queues = plan.fine_queues; a.item_stride = plan.item_stride;
    a.occ_row = plan.occ_row;

    pt_context::Slot& sl = c->slot[slot_index];  // the launch's work buffers are its slot's: another frame may be in flight on the other slot's
    int rc;
    if ((rc = pt_reserve(c, sl.spill, plan.spill)) || (rc = pt_reserve(c, sl.stack_spill, plan.stack_spill)) || (rc = pt_reserve(c, sl.misc, plan.misc)) ||
        (rc = pt_reserve(c, sl.accum, plan.accum)) || (plan.eye_tab && (rc = pt_reserve(c, sl.eye_tab, plan.eye_tab))))
        return rc;
    char* const misc = (char*)sl.misc.p;
    char* const tab = plan.eye_tab ? (char*)sl.eye_tab.p : nullptr;
    a.accum = (double*)sl.accum.p;
    a.eye_tab = (const double*)tab;
    a.spill = (double*)sl.spill.p;
    a.stack_spill = (uint32_t*)sl.stack_spill.p;
    a.work_counter = (unsigned int*)misc;
    a.overflow_flag = (unsigned int*)misc + 1;
    a.counters = (PtCounters*)(misc + 256);
    a.work_queues = (unsigned int*)(misc + 256 + sizeof(PtCounters));
    a.occluders = plan.occ_bytes ? (uint32_t*)(misc + plan.occ_off) : nullptr;
    PT_HIP(c, hipMemsetAsync(misc, 0, plan.misc, stream));
    if (plan.occ_seed != PT_OCC_SEED_NONE) {
        const uint32_t n_occ = (uint32_t)(plan.occ_bytes / 4);
        hipLaunchKernelGGL(pt_occ_seed_kernel, dim3((n_occ + 255) / 256), dim3(256), 0, stream, a.occluders, n_occ, plan.occ_seed == PT_OCC_SEED_HASHED ? 1 : 0, plan.occ_seed_value, plan.occ_all,
                           a.scene.n_nodes);
        PT_HIP(c, hipGetLastError());
        pt_report_occ_seed(n_occ);
    }
    sl.mode = plan.kernel_mode; sl.variant = plan.kernel_variant; sl.counted = stats;
    PT_HIP(c, hipEventRecord(sl.ev0, stream));
    if (a.n_items) {
        const uint32_t n_nodes = (uint32_t)a.scene.n_nodes, node_blocks = (n_nodes + 255) / 256;
        float* const certain = tab ? (float*)(tab + plan.certain_off) : nullptr;
        if (plan.eye_table) {  // (behind ev0: pt_stats.kernel_ms pays for it)
            hipLaunchKernelGGL(pt_eye_table_kernel, dim3(node_blocks), dim3(256), 0, stream, a.scene.inv, (double*)tab, n_nodes, a.cam.eye[0], a.cam.eye[1], a.cam.eye[2]);
            PT_HIP(c, hipGetLastError());
        }
        if (plan.certain_table) {
            hipLaunchKernelGGL(pt_certain_table_kernel, dim3(node_blocks), dim3(256), 0, stream, a.scene.info, a.scene.fwd, a.scene.inv, certain, n_nodes);
            PT_HIP(c, hipGetLastError());
        }
#ifndef PT_NO_DARK_LIGHTS  // (a build without the kernel plans no launch of it)
        if (plan.dark_lights) {  // (reads the table the kernel above fills)
            hipLaunchKernelGGL(pt_dark_light_kernel, dim3((uint32_t)a.scene.n_lights), dim3(256), 0, stream, a.scene.lights, (const float*)certain, (uint32_t*)(misc + plan.dark_off), n_nodes);
            PT_HIP(c, hipGetLastError());
        }
#endif
        if (plan.list_header) {  // behind the eye table's fill, on the launch's stream: the header, then the slot's records
            uint32_t* const records = (uint32_t*)(tab + plan.records_off);
            PT_HIP(c, hipMemsetD32Async((hipDeviceptr_t)(tab + plan.header_off), (int)plan.header_fill, 16, stream));
            if (plan.pixel_lists) {
                const uint32_t tiles = a.n_slots / 64u;
                hipLaunchKernelGGL(pt_pixel_list_kernel, dim3((tiles + PT_PL_BLOCK / 64 - 1) / (PT_PL_BLOCK / 64)), dim3(PT_PL_BLOCK), 0, stream, a, records, plan.list_cap, plan.list_pending,
                                   PT_PL_LISTS | (plan.background_skip ? PT_PL_QUEUE : 0u));
                PT_HIP(c, hipGetLastError());
#if !defined(PT_NO_BACKGROUND_SKIP) && !defined(PT_PL_DEPTH_FIRST)  // (likewise)
                if (plan.background_skip) {
                    hipLaunchKernelGGL(pt_pixel_queue_kernel, dim3((tiles + 255u) / 256u), dim3(256), 0, stream, records, a.n_slots);
                    PT_HIP(c, hipGetLastError());
                }
#endif
            }
        }
        c->last.slot = slot_index; c->last.plan = plan;
        PT_HIP(c, pt_dispatch(a, stats, c->n_cu, stream, &q.grid, true));
        hipLaunchKernelGGL(pt_finish_kernel, dim3((a.n_slots + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), 0, stream, a, plan.background_skip ? 1u : 0u);
        PT_HIP(c, hipGetLastError());
    }
    PT_HIP(c, hipEventRecord(sl.ev1, stream));
    // the overflow flag (always) and the counters (counting build) follow the kernels into the slot's pinned page
    PT_HIP(c, hipMemcpyAsync(sl.host, misc, stats ? PT_SLOT_BYTES : 8, hipMemcpyDeviceToHost, stream));
    PT_HIP(c, hipEventRecord(sl.copy_done, stream));
    return PT_OK;
}

// Reads the overflow flag (always) and, for the counting build, the counters of a finished launch out of its slot's pinned page (the
// caller has waited for the stream: the copy queued behind the kernels is done). A launch in which any lane ran out of traversal
// stack fails with PT_ERR_TRAVERSAL whether or not the caller asked for statistics.
static int pt_collect_stats(pt_context* c, pt_stats* st, int slot_index) {
    pt_context::Slot& sl = c->slot[slot_index];
    if (st) memset(st, 0, sizeof *st);
    unsigned int head[2];  // work counter, overflow flag
    memcpy(head, sl.host, sizeof head);
    if (st) {
        float ms = 0.f;
        PT_HIP(c, hipEventElapsedTime(&ms, sl.ev0, sl.ev1));
        st->kernel_ms = ms;
        if (sl.counted) {
            PtCounters h;
            memcpy(&h, sl.host + 256, sizeof h);
            st->primary = h.primary; st->shadow = h.shadow; st->reflect = h.reflect; st->refract = h.refract;
            st->depth11_skipped = h.depth11_skipped; st->hits = h.hits; st->n_inner = h.n_inner; st->n_leaf = h.n_leaf;
            st->n_analytic = h.n_analytic; st->n_tri = h.n_tri; st->n_bbox = h.n_bbox; st->kd_plane_miss = h.kd_plane_miss;
            st->stack_overflow = h.stack_overflow;
            for (int k = 0; k < 8; k++) st->diag[k] = h.diag[k];
        }
        if (head[1] && !st->stack_overflow) st->stack_overflow = 1;
        st->kernel_mode = sl.mode; st->kernel_variant = sl.variant;
    }
    if (head[1] & 2u) return pt_fail(c, PT_ERR_TRAVERSAL, "fork / join of refracted subtrees stalled (a lane waited for a colour nobody was computing): results invalid");
    if (head[1] & 4u) return pt_fail(c, PT_ERR_TRAVERSAL, "a tree walk did not end (watchdog): results invalid");
    if (head[1]) return pt_fail(c, PT_ERR_TRAVERSAL, "traversal stack overflow");
    return PT_OK;
}

extern "C" int pt_render(pt_context* c, const pt_camera* cam, const double* background, const pt_render_params* p,
                         uint8_t* rgb, double* linear, pt_stats* stats) {
    int rc = pt_check_params(c, cam, p);
    if (rc) return rc;
    if (!background || !rgb) return pt_fail(c, PT_ERR_ARGUMENT, "background and rgb must not be null");
    PT_HIP(c, hipSetDevice(c->device));
    auto t0 = std::chrono::steady_clock::now();
    PtRenderArgs a;
    pt_fill_args(c, cam, p, &a);
    size_t px = (size_t)p->width * p->height;
    size_t bg_bytes = (p->background_rows ? (size_t)p->height : px) * 3 * sizeof(double);
    if ((rc = pt_reserve(c, c->bg, bg_bytes)) || (rc = pt_reserve(c, c->rgb, px * 3))) return rc;
    if (linear && (rc = pt_reserve(c, c->linear, px * 3 * sizeof(double)))) return rc;
    PT_HIP(c, hipMemcpy(c->bg.p, background, bg_bytes, hipMemcpyHostToDevice));
    // pixels outside the slice / of other ranks keep the caller's bytes (render.rs:135-138)
    PT_HIP(c, hipMemcpy(c->rgb.p, rgb, px * 3, hipMemcpyHostToDevice));
    if (linear) PT_HIP(c, hipMemcpy(c->linear.p, linear, px * 3 * sizeof(double), hipMemcpyHostToDevice));
    a.background = (const double*)c->bg.p;
    a.compact = 0;
    a.rgb = (uint8_t*)c->rgb.p;
    a.linear = linear ? (double*)c->linear.p : nullptr;
    bool counted = p->collect_stats != 0;
    const int slot_index = c->slot_next;
    if ((rc = pt_render_common(c, a, counted, nullptr))) return rc;
    PT_HIP(c, hipDeviceSynchronize());
    PT_HIP(c, hipMemcpy(rgb, c->rgb.p, px * 3, hipMemcpyDeviceToHost));
    if (linear) PT_HIP(c, hipMemcpy(linear, c->linear.p, px * 3 * sizeof(double), hipMemcpyDeviceToHost));
    rc = pt_collect_stats(c, stats, slot_index);
    if (stats) stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

extern "C" int pt_render_device(pt_context* c, const pt_camera* cam, const double* d_background, const pt_render_params* p,
                                int compact, void* d_rgb, void* hip_stream) {
    int rc = pt_check_params(c, cam, p);
    if (rc) return rc;
    if (!d_background || !d_rgb) return pt_fail(c, PT_ERR_ARGUMENT, "d_background and d_rgb must not be null");
    PT_HIP(c, hipSetDevice(c->device));
    PtRenderArgs a;
    pt_fill_args(c, cam, p, &a);
    a.background = d_background;
    a.compact = compact ? 1 : 0;
    a.rgb = (uint8_t*)d_rgb;
    a.linear = nullptr;
    const int slot_index = c->slot_next;
    if (c->slot[slot_index].pending) return pt_fail(c, PT_ERR_ARGUMENT, "too many renders in flight on this context: pt_render_finish first");
    c->slot[slot_index].t_start = std::chrono::steady_clock::now();
    if ((rc = pt_render_common(c, a, p->collect_stats != 0, (hipStream_t)hip_stream, slot_index))) return rc;
    c->slot[slot_index].pending = true;
    c->slot_next = (slot_index + 1) % pt_context::PT_SLOTS;
    return PT_OK;
}

extern "C" int pt_render_finish(pt_context* c, pt_stats* stats) {
    if (!c) return PT_ERR_ARGUMENT;
    const int slot_index = c->slot_oldest;
    pt_context::Slot& sl = c->slot[slot_index];
    if (!sl.pending) return pt_fail(c, PT_ERR_ARGUMENT, "no render in flight");
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipEventSynchronize(sl.copy_done));  // behind the kernels, ev1 and the copy of the flag / the counters
    sl.pending = false;
    c->slot_oldest = (slot_index + 1) % pt_context::PT_SLOTS;
    int rc = pt_collect_stats(c, stats, slot_index);
    if (stats) stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - sl.t_start).count();
    return rc;
}

extern "C" int pt_untile_device(pt_context* c, const pt_render_params* p, const void* d_gathered, void* d_rgb, void* hip_stream) {
    if (!c || !p || !d_gathered || !d_rgb) return PT_ERR_ARGUMENT;
    if (p->width == 0 || p->height == 0 || p->tile_ranks == 0) return pt_fail(c, PT_ERR_ARGUMENT, "bad params");
    if (p->slice.x0 >= p->width || p->slice.x1 >= p->width || p->slice.y0 >= p->height || p->slice.y1 >= p->height)
        return pt_fail(c, PT_ERR_SLICE, "slice corner outside the image (render.rs:79-90)");
    if (p->slice.x1 < p->slice.x0 || p->slice.y1 < p->slice.y0) return PT_OK;
    PT_HIP(c, hipSetDevice(c->device));
    PtRenderArgs a;
    memset(&a, 0, sizeof a);
    a.width = p->width; a.height = p->height;
    a.x0 = p->slice.x0; a.y0 = p->slice.y0; a.x1 = p->slice.x1; a.y1 = p->slice.y1;
    a.tile_ranks = p->tile_ranks;
    uint32_t per = pt_slots_per_rank(p);
    uint32_t total = per * p->tile_ranks;
    hipLaunchKernelGGL(pt_untile_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, a, per, (const uint8_t*)d_gathered, (uint8_t*)d_rgb);
    PT_HIP(c, hipGetLastError());
    return PT_OK;
}

static bool pt_params_to_args(const pt_render_params* p, uint32_t rank, PtRenderArgs* a) {
    if (!p || p->width == 0 || p->height == 0 || p->tile_ranks == 0 || rank >= p->tile_ranks) return false;
    if (p->slice.x0 >= p->width || p->slice.x1 >= p->width || p->slice.y0 >= p->height || p->slice.y1 >= p->height) return false;
    memset(a, 0, sizeof *a);
    a->width = p->width; a->height = p->height;
    a->x0 = p->slice.x0; a->y0 = p->slice.y0; a->x1 = p->slice.x1; a->y1 = p->slice.y1;
    a->tile_rank = rank; a->tile_ranks = p->tile_ranks;
    return true;
}

extern "C" int pt_tile_slot_pixel(const pt_render_params* p, uint32_t rank, uint32_t slot, uint32_t* x, uint32_t* y) {
    PtRenderArgs a;
    if (!x || !y || !pt_params_to_args(p, rank, &a)) return PT_ERR_ARGUMENT;
    if (p->slice.x1 < p->slice.x0 || p->slice.y1 < p->slice.y0 || slot >= pt_slots_per_rank(p)) return 0;
    return pt_slot_to_pixel(a, slot, x, y) ? 1 : 0;
}

extern "C" int pt_untile_host(const pt_render_params* p, const uint8_t* gathered, uint8_t* rgb) {
    PtRenderArgs a;
    if (!gathered || !rgb || !pt_params_to_args(p, 0, &a)) return PT_ERR_ARGUMENT;
    if (p->slice.x1 < p->slice.x0 || p->slice.y1 < p->slice.y0) return PT_OK;
    uint32_t per = pt_slots_per_rank(p);
    for (uint32_t r = 0; r < p->tile_ranks; r++) {
        a.tile_rank = r;
        for (uint32_t w = 0; w < per; w++) {
            uint32_t x, y;
            if (!pt_slot_to_pixel(a, w, &x, &y)) continue;
            const uint8_t* s = gathered + 3 * ((size_t)r * per + w);
            uint8_t* d = rgb + 3 * ((size_t)y * p->width + x);
            d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
        }
    }
    return PT_OK;
}

// ------------------------------------------------------------------------------------------------
// Primary visibility (pt_aov.h)
// ------------------------------------------------------------------------------------------------
static hipError_t pt_aov_dispatch(const PtAovArgs& a, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    PT_MODE_LAUNCH(pt_aov_launch_mode_, a.r.scene.mode, a, n_cu, stream, grid, launch)
}

// What refuses a second pass on the pass object pt_aov, pt_guides and pt_chart share: the open one's kind and the call that closes it.
static const char* pt_aov_open_words(const pt_context* c) {
    if (c->aov.chart) return "a pt_chart_device pass is in flight: pt_aov_finish first";
    return c->aov.guides ? "a pt_guides_device pass is in flight: pt_guides_finish first" : "a pt_aov_device pass is in flight: pt_aov_finish first";
}

// Everything that can be refused without a HIP call, in the order the header gives.
static int pt_aov_check(pt_context* c, const pt_camera* cam, const pt_aov_params* p, const pt_aov_buffers* out) {
    if (!c || !cam || !p) return PT_ERR_ARGUMENT;
    if (!out || !(out->depth || out->position || out->normal || out->node || out->sub || out->material))
        return pt_fail(c, PT_ERR_ARGUMENT, "pt_aov: no output buffer asked for");
    if (!std::isfinite(p->offset[0]) || !std::isfinite(p->offset[1])) return pt_fail(c, PT_ERR_ARGUMENT, "pt_aov: offset must be finite");
    if (!c->have_scene) return pt_fail(c, PT_ERR_NO_SCENE, "no scene uploaded");
    if (p->width == 0 || p->height == 0) return pt_fail(c, PT_ERR_ARGUMENT, "width and height must be positive");
    if (p->slice.x0 >= p->width || p->slice.x1 >= p->width || p->slice.y0 >= p->height || p->slice.y1 >= p->height)
        return pt_fail(c, PT_ERR_SLICE, "slice corner outside the image (render.rs:79-90)");
    if (c->aov.pass.pending) return pt_fail(c, PT_ERR_ARGUMENT, pt_aov_open_words(c));
    return PT_OK;
}

// Queues the pass on `stream` (pt_pass_open ... pt_pass_seal): the kernel between the pass's two events, launched only where the slice holds a tile.
// `out` holds DEVICE pointers. Deeper entries of a lane's stack than its LDS area holds (pt_walk_sizing) go to its HBM column.
static int pt_aov_common(pt_context* c, const pt_camera* cam, const pt_aov_params* p, const pt_aov_buffers& out, hipStream_t stream) {
    PtPass& v = c->aov.pass;
    int rc = pt_pass_prepare(c, v);
    if (rc) return rc;
    pt_render_params rp;
    memset(&rp, 0, sizeof rp);
    rp.width = p->width; rp.height = p->height; rp.slice = p->slice;
    rp.samples = 1; rp.sample_mode = PT_SAMPLE_CENTRE; rp.tile_rank = 0; rp.tile_ranks = 1;
    PtAovArgs a;
    pt_fill_args(c, cam, &rp, &a.r);  // samples = 1: one work item per 8x8 tile of the slice
    a.off_x = p->offset[0]; a.off_y = p->offset[1];
    a.depth = out.depth; a.position = out.position; a.normal = out.normal; a.node = out.node; a.sub = out.sub; a.material = out.material;
    pt_walk_sizing(a.r, pt_aov_waves(a.r.scene.mode));
    uint32_t grid = 0;
    PT_HIP(c, pt_aov_dispatch(a, c->n_cu, stream, &grid, false));
    if ((rc = pt_pass_open(c, v, a.r, grid, false, stream))) return rc;
    if (a.r.n_items) PT_HIP(c, pt_aov_dispatch(a, c->n_cu, stream, &grid, true));
    return pt_pass_seal(c, v);
}

extern "C" int pt_aov(pt_context* c, const pt_camera* cam, const pt_aov_params* p, const pt_aov_buffers* host_out, double* kernel_ms) {
    int rc = pt_aov_check(c, cam, p, host_out);
    if (rc) return rc;
    PT_HIP(c, hipSetDevice(c->device));
    const size_t px = (size_t)p->width * p->height;
    PtBuf* out = c->aov.out;
    PtStage s[6] = {pt_stage_output(host_out->depth, out[0], px * 8), pt_stage_output(host_out->position, out[1], px * 24), pt_stage_output(host_out->normal, out[2], px * 24),
                    pt_stage_output(host_out->node, out[3], px * 4), pt_stage_output(host_out->sub, out[4], px * 4), pt_stage_output(host_out->material, out[5], px * 4)};
    if ((rc = pt_stage_in(c, s))) return rc;
    const pt_aov_buffers d_out = {(double*)s[0].dev, (double*)s[1].dev, (double*)s[2].dev, (int32_t*)s[3].dev, (int32_t*)s[4].dev, (int32_t*)s[5].dev};
    return pt_stage_out(c, c->aov.pass, pt_aov_common(c, cam, p, d_out, nullptr), s, kernel_ms, p);  // (only the slice's rectangle comes back)
}

extern "C" int pt_aov_device(pt_context* c, const pt_camera* cam, const pt_aov_params* p, const pt_aov_buffers* device_out, void* hip_stream) {
    int rc = pt_aov_check(c, cam, p, device_out);
    if (rc) return rc;
    PT_HIP(c, hipSetDevice(c->device));
    c->aov.guides = false; c->aov.chart = false;
    return pt_pass_device_tail(c, c->aov.pass, pt_aov_common(c, cam, p, *device_out, (hipStream_t)hip_stream));
}

extern "C" int pt_aov_finish(pt_context* c, double* kernel_ms) {
    if (!c) return PT_ERR_ARGUMENT;
    return pt_pass_finish(c, c->aov.pass, "no pt_aov_device pass in flight", kernel_ms);  // (also what pt_guides_finish says: the same function)
}

// ------------------------------------------------------------------------------------------------
// Guides (pt_guides.h): the primary-visibility pass with the albedo, on that pass's PtPass
// ------------------------------------------------------------------------------------------------
static hipError_t pt_guides_dispatch(const PtGuidesArgs& a, bool tex, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    PT_MODE_LAUNCH(pt_guides_launch_mode_, a.r.scene.mode, a, tex, n_cu, stream, grid, launch)
}

// Everything that can be refused without a HIP call: pt_aov_check's list, in its order.
static int pt_guides_check(pt_context* c, const pt_camera* cam, const pt_aov_params* p, const pt_guides_buffers* out) {
    if (!c || !cam || !p) return PT_ERR_ARGUMENT;
    if (!out || !(out->albedo || out->position || out->normal || out->node)) return pt_fail(c, PT_ERR_ARGUMENT, "pt_guides: no output buffer asked for");
    if (!std::isfinite(p->offset[0]) || !std::isfinite(p->offset[1])) return pt_fail(c, PT_ERR_ARGUMENT, "pt_guides: offset must be finite");
    if (!c->have_scene) return pt_fail(c, PT_ERR_NO_SCENE, "no scene uploaded");
    if (p->width == 0 || p->height == 0) return pt_fail(c, PT_ERR_ARGUMENT, "width and height must be positive");
    if (p->slice.x0 >= p->width || p->slice.x1 >= p->width || p->slice.y0 >= p->height || p->slice.y1 >= p->height)
        return pt_fail(c, PT_ERR_SLICE, "slice corner outside the image (render.rs:79-90)");
    if (c->aov.pass.pending) return pt_fail(c, PT_ERR_ARGUMENT, pt_aov_open_words(c));
    return PT_OK;
}

// Queues the pass on `stream`, as pt_aov_common does and on its PtPass. `out` holds DEVICE pointers. A scene with material maps launches the TEX instantiation.
static int pt_guides_common(pt_context* c, const pt_camera* cam, const pt_aov_params* p, const pt_guides_buffers& out, hipStream_t stream) {
    PtPass& v = c->aov.pass;
    int rc = pt_pass_prepare(c, v);
    if (rc) return rc;
    pt_render_params rp;
    memset(&rp, 0, sizeof rp);
    rp.width = p->width; rp.height = p->height; rp.slice = p->slice;
    rp.samples = 1; rp.sample_mode = PT_SAMPLE_CENTRE; rp.tile_rank = 0; rp.tile_ranks = 1;
    PtGuidesArgs a;
    pt_fill_args(c, cam, &rp, &a.r);  // samples = 1: one work item per 8x8 tile of the slice
    a.off_x = p->offset[0]; a.off_y = p->offset[1];
    a.albedo = out.albedo; a.position = out.position; a.normal = out.normal; a.node = out.node;
    pt_walk_sizing(a.r, pt_aov_waves(a.r.scene.mode));
    const bool tex = a.r.scene.mat_maps != nullptr;
    uint32_t grid = 0;
    PT_HIP(c, pt_guides_dispatch(a, tex, c->n_cu, stream, &grid, false));
    if ((rc = pt_pass_open(c, v, a.r, grid, false, stream))) return rc;
    if (a.r.n_items) PT_HIP(c, pt_guides_dispatch(a, tex, c->n_cu, stream, &grid, true));
    return pt_pass_seal(c, v);
}

extern "C" int pt_guides(pt_context* c, const pt_camera* cam, const pt_aov_params* p, const pt_guides_buffers* host_out, double* kernel_ms) {
    int rc = pt_guides_check(c, cam, p, host_out);
    if (rc) return rc;
    PT_HIP(c, hipSetDevice(c->device));
    const size_t px = (size_t)p->width * p->height;
    PtStage s[4] = {pt_stage_output(host_out->albedo, c->aov.albedo, px * 24), pt_stage_output(host_out->position, c->aov.out[1], px * 24),
                    pt_stage_output(host_out->normal, c->aov.out[2], px * 24), pt_stage_output(host_out->node, c->aov.out[3], px * 4)};
    if ((rc = pt_stage_in(c, s))) return rc;
    const pt_guides_buffers d_out = {(double*)s[0].dev, (double*)s[1].dev, (double*)s[2].dev, (int32_t*)s[3].dev};
    return pt_stage_out(c, c->aov.pass, pt_guides_common(c, cam, p, d_out, nullptr), s, kernel_ms, p);  // (only the slice's rectangle comes back, as in pt_aov)
}

extern "C" int pt_guides_device(pt_context* c, const pt_camera* cam, const pt_aov_params* p, const pt_guides_buffers* device_out, void* hip_stream) {
    int rc = pt_guides_check(c, cam, p, device_out);
    if (rc) return rc;
    PT_HIP(c, hipSetDevice(c->device));
    c->aov.guides = true; c->aov.chart = false;
    return pt_pass_device_tail(c, c->aov.pass, pt_guides_common(c, cam, p, *device_out, (hipStream_t)hip_stream));
}

// The pass is pt_aov's: one function closes either.
extern "C" int pt_guides_finish(pt_context* c, double* kernel_ms) { return pt_aov_finish(c, kernel_ms); }

// ------------------------------------------------------------------------------------------------
// Chart (pt_chart.h: the contract; pt_chart.hip: the kernels): a mesh's light-map texels as surface points, on the primary-visibility pass's PtPass
// ------------------------------------------------------------------------------------------------
// What concerns the node, in the order the header gives; the context has a scene. mesh_out: the node's mesh.
static int pt_chart_node_check(pt_context* c, uint32_t node, uint32_t* mesh_out) {
    const pt_context::Resident& res = c->res;
    if (node >= res.n_nodes) return pt_fail(c, PT_ERR_ARGUMENT, "pt_chart: node " + std::to_string(node) + " of " + std::to_string(res.n_nodes) + " flattened nodes");
    const uint32_t type = res.info[4 * (size_t)node];
    if (type != PT_PRIM_MESH && type != PT_PRIM_KDMESH) return pt_fail(c, PT_ERR_ARGUMENT, "pt_chart: node " + std::to_string(node) + " is no mesh (PT_PRIM_MESH, PT_PRIM_KDMESH)");
    *mesh_out = res.info[4 * (size_t)node + 1];
    return PT_OK;
}

// Everything that can be refused without a HIP call, in the order the header gives. (pt_fail takes a NULL context.)
static int pt_chart_check(pt_context* c, const pt_chart_params* p, const double* uv, const pt_chart_buffers* out, uint32_t* mesh_out) {
    if (!c || !p || !out) return pt_fail(c, PT_ERR_ARGUMENT, "pt_chart: NULL context, params or buffers");
    if (!(out->position || out->normal || out->tri || out->covered)) return pt_fail(c, PT_ERR_ARGUMENT, "pt_chart: no output buffer asked for");
    if (p->flags & ~PT_CHART_FLIP_NORMAL) return pt_fail(c, PT_ERR_ARGUMENT, "pt_chart: unknown flags");
    if (p->width == 0 || p->height == 0) return pt_fail(c, PT_ERR_ARGUMENT, "pt_chart: width and height must be positive");
    if ((uint64_t)p->width * p->height > PT_AO_MAX) return pt_fail(c, PT_ERR_ARGUMENT, "pt_chart: more than PT_AO_MAX texels");
    if (!c->have_scene) return pt_fail(c, PT_ERR_NO_SCENE, "no scene uploaded");
    if (int rc = pt_chart_node_check(c, p->node, mesh_out)) return rc;
    if (!uv && !(c->view.tri_uv && c->res.place[*mesh_out].has_uv))
        return pt_fail(c, PT_ERR_ARGUMENT, c->view.tri_uv ? "pt_chart: uv is NULL and the node's mesh has no texture coordinates of its own (mesh_has_texcoords)"
                                                          : "pt_chart: uv is NULL and the scene keeps no texture coordinates on the device (no material has a texture or a normal map)");
    if (c->aov.pass.pending) return pt_fail(c, PT_ERR_ARGUMENT, pt_aov_open_words(c));
    return PT_OK;
}

extern "C" int pt_chart_triangles(pt_context* c, uint32_t node, uint64_t* n_tris) {
    if (!c || !n_tris) return pt_fail(c, PT_ERR_ARGUMENT, "pt_chart_triangles: NULL context or n_tris");
    if (!c->have_scene) return pt_fail(c, PT_ERR_NO_SCENE, "no scene uploaded");
    uint32_t mesh = 0;
    if (int rc = pt_chart_node_check(c, node, &mesh)) return rc;
    *n_tris = c->res.meshes[mesh].tri_count;
    return PT_OK;
}

// Which of the kernels a pass queues: all three. PORTRAYER_CHART_PHASES=1 (seed and own) or 2 (resolve, over the owner map the call before left) lets
// profiles/chart/measure.py time them apart.
static int pt_chart_phases() {
    if (const char* e = getenv("PORTRAYER_CHART_PHASES")) {
        const int w = atoi(e);
        if (w == 1 || w == 2) return w;
    }
    return 3;
}

// Queues the pass on `stream` (pt_pass_open ... pt_pass_seal) on pt_aov's PtPass. d_uv null: the mesh's own coordinates in tri_uv. `out` holds DEVICE pointers.
// No tree is walked: the pass opens with an empty launch (no lanes, no stack columns) for the events and the protocol alone.
static int pt_chart_common(pt_context* c, const pt_chart_params* p, uint32_t mesh, const double* d_uv, const pt_chart_buffers& out, hipStream_t stream) {
    PtPass& v = c->aov.pass;
    int rc = pt_pass_prepare(c, v);
    if (rc) return rc;
    if ((rc = pt_reserve(c, c->aov.chart_owner, (size_t)p->width * p->height * 4))) return rc;
    const PtMeshInfo& mi = c->res.meshes[mesh];
    const bool smooth = (c->res.info[4 * (size_t)p->node + 2] & 1u) != 0 && c->view.tri_n != nullptr;  // (pt_hit_model's choice; the upload refuses a smooth node without normals)
    PtChartArgs a;
    memset(&a, 0, sizeof a);
    a.width = p->width; a.height = p->height; a.flags = p->flags; a.n_tris = mi.tri_count;
    a.uv = d_uv ? d_uv : c->view.tri_uv + 6 * (size_t)mi.tri_first;
    a.tri_v = c->view.tri_v + 9 * (size_t)mi.tri_first;
    a.tri_n = smooth ? c->view.tri_n + 9 * (size_t)mi.tri_first : nullptr;
    a.fwd = c->view.fwd + 12 * (size_t)p->node; a.nrm = c->view.nrm + 9 * (size_t)p->node;
    a.owner = (uint32_t*)c->aov.chart_owner.p;
    a.position = out.position; a.normal = out.normal; a.tri = out.tri; a.covered = out.covered;
    PtRenderArgs r;
    memset(&r, 0, sizeof r);
    r.scene = c->view;
    if ((rc = pt_pass_open(c, v, r, 0, false, stream))) return rc;
    PT_HIP(c, pt_chart_launch(a, pt_chart_phases(), stream));
    return pt_pass_seal(c, v);
}

extern "C" int pt_chart(pt_context* c, const pt_chart_params* p, const double* uv, const pt_chart_buffers* host_out, double* kernel_ms) {
    uint32_t mesh = 0;
    int rc = pt_chart_check(c, p, uv, host_out, &mesh);
    if (rc) return rc;
    PT_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)p->width * p->height, n_tris = c->res.meshes[mesh].tri_count;
    PtStage s[5] = {pt_stage_output(host_out->position, c->aov.out[1], n * 24), pt_stage_output(host_out->normal, c->aov.out[2], n * 24),
                    pt_stage_output(host_out->tri, c->aov.out[3], n * 4), pt_stage_output(host_out->covered, c->aov.chart_covered, n),
                    pt_stage_input(uv, c->aov.chart_uv, n_tris * 48)};  // (uv null: the row is absent, and d_uv null)
    if ((rc = pt_stage_in(c, s))) return rc;
    const pt_chart_buffers d_out = {(double*)s[0].dev, (double*)s[1].dev, (int32_t*)s[2].dev, (uint8_t*)s[3].dev};
    return pt_stage_out(c, c->aov.pass, pt_chart_common(c, p, mesh, (const double*)s[4].dev, d_out, nullptr), s, kernel_ms);
}

extern "C" int pt_chart_device(pt_context* c, const pt_chart_params* p, const double* d_uv, const pt_chart_buffers* device_out, void* hip_stream) {
    uint32_t mesh = 0;
    int rc = pt_chart_check(c, p, d_uv, device_out, &mesh);
    if (rc) return rc;
    PT_HIP(c, hipSetDevice(c->device));
    // the caller's pointers, before anything is queued: device memory of this device, and long enough
    const uint64_t n = (uint64_t)p->width * p->height, n_tris = c->res.meshes[mesh].tri_count;
    if (d_uv && n_tris && (rc = pt_check_device_pointer(c, d_uv, n_tris * 48, "pt_chart_device: d_uv"))) return rc;
    if (device_out->position && (rc = pt_check_device_pointer(c, device_out->position, n * 24, "pt_chart_device: position"))) return rc;
    if (device_out->normal && (rc = pt_check_device_pointer(c, device_out->normal, n * 24, "pt_chart_device: normal"))) return rc;
    if (device_out->tri && (rc = pt_check_device_pointer(c, device_out->tri, n * 4, "pt_chart_device: tri"))) return rc;
    if (device_out->covered && (rc = pt_check_device_pointer(c, device_out->covered, n, "pt_chart_device: covered"))) return rc;
    c->aov.guides = false; c->aov.chart = true;
    return pt_pass_device_tail(c, c->aov.pass, pt_chart_common(c, p, mesh, d_uv, *device_out, (hipStream_t)hip_stream));
}

// ------------------------------------------------------------------------------------------------
// Ray queries (pt_rays.h)
// ------------------------------------------------------------------------------------------------
static hipError_t pt_rays_dispatch(const PtRaysArgs& a, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    PT_MODE_LAUNCH(pt_rays_launch_mode_, a.r.scene.mode, a, n_cu, stream, grid, launch)
}

// The bounded-segment form of the pass (pt_segments.h): the same arguments and a bound per ray.
static hipError_t pt_segments_dispatch(const PtSegmentsArgs& a, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    PT_MODE_LAUNCH(pt_segments_launch_mode_, a.q.r.scene.mode, a, n_cu, stream, grid, launch)
}

// Everything that can be refused without a HIP call, in the order the header gives. (pt_fail takes a NULL context.)
static int pt_rays_check(pt_context* c, const pt_rays_params* p, const double* origins, const double* directions, const pt_rays_buffers* out) {
    if (!c || !p || !origins || !directions) return pt_fail(c, PT_ERR_ARGUMENT, "pt_rays: NULL context, params, origins or directions");
    if (!out || !(out->t || out->position || out->normal || out->node || out->sub || out->material || out->occluded))
        return pt_fail(c, PT_ERR_ARGUMENT, "pt_rays: no output buffer asked for");
    if (p->n > PT_RAYS_MAX) return pt_fail(c, PT_ERR_ARGUMENT, "pt_rays: more than PT_RAYS_MAX rays in one call");
    if ((p->any_hit != 0 && p->any_hit != 1) || (p->reorder != 0 && p->reorder != 1)) return pt_fail(c, PT_ERR_ARGUMENT, "pt_rays: any_hit and reorder are 0 or 1");
    if (p->any_hit && (out->t || out->position || out->normal || out->node || out->sub || out->material))
        return pt_fail(c, PT_ERR_ARGUMENT, "pt_rays: an occlusion query (any_hit = 1) answers `occluded` only");
    if (!c->have_scene) return pt_fail(c, PT_ERR_NO_SCENE, "no scene uploaded");
    if (c->rays.pass.pending) return pt_fail(c, PT_ERR_ARGUMENT, "a pt_rays_device / pt_segments_device pass is in flight: pt_rays_finish first");
    return PT_OK;
}

// pt_segments': pt_rays' and the bound.
static int pt_segments_check(pt_context* c, const pt_rays_params* p, const double* origins, const double* directions, const double* t_max, const pt_rays_buffers* out) {
    if (!c || !p || !origins || !directions || !t_max) return pt_fail(c, PT_ERR_ARGUMENT, "pt_segments: NULL context, params, origins, directions or t_max");
    return pt_rays_check(c, p, origins, directions, out);
}

// reorder = 1: the buffers for n rays, and *perm (slot -> ray index) pointed at where the sort will leave it ...
static int pt_ray_sort_reserve(pt_context* c, PtRaySort& s, uint64_t n, const uint32_t** perm) {
    PT_HIP(c, pt_rays_sort_bytes(n, &s.tmp_bytes));
    int rc;
    if ((rc = pt_reserve(c, s.keys[0], n * 8)) || (rc = pt_reserve(c, s.keys[1], n * 8)) || (rc = pt_reserve(c, s.vals[0], n * 4)) || (rc = pt_reserve(c, s.vals[1], n * 4)) ||
        (rc = pt_reserve(c, s.tmp, s.tmp_bytes)))
        return rc;
    *perm = (const uint32_t*)s.vals[1].p;
    return PT_OK;
}
// ... and the keying and the sort on `stream`, behind the pass's first event.
static int pt_ray_sort_queue(pt_context* c, PtRaySort& s, uint64_t n, const double* d_origins, const double* d_directions, hipStream_t stream) {
    PT_HIP(c, pt_rays_sort(n, d_origins, d_directions, c->root_lo, c->root_hi, (unsigned long long*)s.keys[0].p, (unsigned long long*)s.keys[1].p, (uint32_t*)s.vals[0].p,
                           (uint32_t*)s.vals[1].p, s.tmp.p, s.tmp_bytes, stream));
    return PT_OK;
}

// Queues the pass on `stream` (pt_pass_open ... pt_pass_seal): between the pass's two events the keying and the sort (reorder = 1) and the cast kernel.
// Every pointer is a DEVICE pointer. The LDS stack area is sized as for the primary-visibility pass (pt_walk_sizing).
// d_t_max: null = pt_rays' kernel; else the bounded-segment kernel (pt_segments), which takes the same arguments and that array.
static int pt_rays_common(pt_context* c, const pt_rays_params* p, const double* d_origins, const double* d_directions, const pt_rays_buffers& out, hipStream_t stream,
                          const double* d_t_max = nullptr) {
    PtPass& v = c->rays.pass;
    int rc = pt_pass_prepare(c, v);
    if (rc) return rc;
    PtRaysArgs a;
    memset(&a, 0, sizeof a);
    a.r.scene = c->view;
    a.r.n_items = (uint32_t)((p->n + 63u) / 64u);  // (n <= PT_RAYS_MAX = 2^30)
    a.n = p->n; a.origins = d_origins; a.directions = d_directions; a.any = p->any_hit;
    a.t = out.t; a.position = out.position; a.normal = out.normal; a.node = out.node; a.sub = out.sub; a.material = out.material; a.occluded = out.occluded;
    pt_walk_sizing(a.r, pt_rays_waves(a.r.scene.mode));
    uint32_t grid = 0;
    auto dispatch = [&](bool launch) -> hipError_t {  // (the segments kernel's argument block is built from `a` as it stands at the call)
        if (!d_t_max) return pt_rays_dispatch(a, c->n_cu, stream, &grid, launch);
        PtSegmentsArgs s;
        s.q = a; s.t_max = d_t_max;
        return pt_segments_dispatch(s, c->n_cu, stream, &grid, launch);
    };
    PT_HIP(c, dispatch(false));
    if (p->reorder && (rc = pt_ray_sort_reserve(c, c->rays.sort, p->n, &a.perm))) return rc;
    if ((rc = pt_pass_open(c, v, a.r, grid, false, stream))) return rc;
    if (p->reorder && (rc = pt_ray_sort_queue(c, c->rays.sort, p->n, d_origins, d_directions, stream))) return rc;
    PT_HIP(c, dispatch(true));
    return pt_pass_seal(c, v);
}

// The host-buffer path of pt_rays (t_max null) and pt_segments: upload, pass, copy back.
static int pt_rays_host(pt_context* c, const pt_rays_params* p, const double* origins, const double* directions, const double* t_max, const pt_rays_buffers* host_out, double* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0;
    if (p->n == 0) return PT_OK;
    PT_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)p->n;
    pt_context::Rays& v = c->rays;
    PtStage s[10] = {pt_stage_input(origins, v.in[0], n * 24), pt_stage_input(directions, v.in[1], n * 24), pt_stage_input(t_max, v.in_t_max, n * 8),  // (pt_rays: no t_max row)
                     pt_stage_output(host_out->t, v.out[0], n * 8), pt_stage_output(host_out->position, v.out[1], n * 24), pt_stage_output(host_out->normal, v.out[2], n * 24),
                     pt_stage_output(host_out->node, v.out[3], n * 4), pt_stage_output(host_out->sub, v.out[4], n * 4), pt_stage_output(host_out->material, v.out[5], n * 4),
                     pt_stage_output(host_out->occluded, v.out[6], n)};
    if (int rc = pt_stage_in(c, s)) return rc;
    const pt_rays_buffers d_out = {(double*)s[3].dev, (double*)s[4].dev, (double*)s[5].dev, (int32_t*)s[6].dev, (int32_t*)s[7].dev, (int32_t*)s[8].dev, (uint8_t*)s[9].dev};
    return pt_stage_out(c, v.pass, pt_rays_common(c, p, (const double*)s[0].dev, (const double*)s[1].dev, d_out, nullptr, (const double*)s[2].dev), s, kernel_ms);
}

// ... and the device-buffer path of both.
static int pt_rays_queue(pt_context* c, const pt_rays_params* p, const double* d_origins, const double* d_directions, const double* d_t_max, const pt_rays_buffers* device_out, void* hip_stream) {
    if (p->n == 0) return PT_OK;  // nothing queued, nothing to finish
    PT_HIP(c, hipSetDevice(c->device));
    return pt_pass_device_tail(c, c->rays.pass, pt_rays_common(c, p, d_origins, d_directions, *device_out, (hipStream_t)hip_stream, d_t_max));
}

extern "C" int pt_rays(pt_context* c, const pt_rays_params* p, const double* origins, const double* directions, const pt_rays_buffers* host_out, double* kernel_ms) {
    int rc = pt_rays_check(c, p, origins, directions, host_out);
    if (rc) return rc;
    return pt_rays_host(c, p, origins, directions, nullptr, host_out, kernel_ms);
}

extern "C" int pt_rays_device(pt_context* c, const pt_rays_params* p, const double* d_origins, const double* d_directions, const pt_rays_buffers* device_out, void* hip_stream) {
    int rc = pt_rays_check(c, p, d_origins, d_directions, device_out);
    if (rc) return rc;
    return pt_rays_queue(c, p, d_origins, d_directions, nullptr, device_out, hip_stream);
}

extern "C" int pt_segments(pt_context* c, const pt_rays_params* p, const double* origins, const double* directions, const double* t_max, const pt_rays_buffers* host_out, double* kernel_ms) {
    int rc = pt_segments_check(c, p, origins, directions, t_max, host_out);
    if (rc) return rc;
    return pt_rays_host(c, p, origins, directions, t_max, host_out, kernel_ms);
}

extern "C" int pt_segments_device(pt_context* c, const pt_rays_params* p, const double* d_origins, const double* d_directions, const double* d_t_max, const pt_rays_buffers* device_out, void* hip_stream) {
    int rc = pt_segments_check(c, p, d_origins, d_directions, d_t_max, device_out);
    if (rc) return rc;
    return pt_rays_queue(c, p, d_origins, d_directions, d_t_max, device_out, hip_stream);
}

extern "C" int pt_rays_finish(pt_context* c, double* kernel_ms) {
    if (!c) return PT_ERR_ARGUMENT;
    return pt_pass_finish(c, c->rays.pass, "no pt_rays_device / pt_segments_device pass in flight", kernel_ms);
}

// ------------------------------------------------------------------------------------------------
// Ambient occlusion (pt_ao.h: the contract; pt_ao_inst.hip: the kernel): a ray-query pass, on that pass's PtPass
// ------------------------------------------------------------------------------------------------
static hipError_t pt_ao_dispatch(const PtAoArgs& a, int layout, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    PT_MODE_LAUNCH(pt_ao_launch_mode_, a.r.scene.mode, a, layout, n_cu, stream, grid, launch)
}

// What pt_ao refuses of a parameter block, in the order the header gives; null: nothing. (Also pt_test_ao_rays_host's check.)
static const char* pt_ao_params_error(const pt_ao_params* p) {
    if (p->n > PT_AO_MAX) return "pt_ao: more than PT_AO_MAX points in one call";
    if (p->samples == 0 || p->samples > 64 || (p->samples & (p->samples - 1)) != 0) return "pt_ao: samples must be a power of two, 1 .. 64";
    if (!(p->radius > PT_EPSILON)) return "pt_ao: radius must be greater than EPSILON (+inf is allowed)";
    if (!std::isfinite(p->bias) || p->bias < 0.0) return "pt_ao: bias must be finite and not negative";
    if (p->flags & ~PT_AO_FACE_EYE) return "pt_ao: unknown flags";
    if ((p->flags & PT_AO_FACE_EYE) && !(std::isfinite(p->eye[0]) && std::isfinite(p->eye[1]) && std::isfinite(p->eye[2]))) return "pt_ao: PT_AO_FACE_EYE needs a finite eye";
    return nullptr;
}

// What steps 1 to 8 read of a parameter block, pt_ao's or pt_gather's (the eye only with PT_AO_FACE_EYE).
template <class Params>
static PtAoSet pt_ao_set(const Params* p) {
    PtAoSet s;
    s.seed = p->seed; s.first_index = p->first_index; s.pass = p->pass; s.flags = p->flags; s.bias = p->bias;
    s.eye = (p->flags & PT_AO_FACE_EYE) ? pt_v3(p->eye[0], p->eye[1], p->eye[2]) : pt_v3(0.0, 0.0, 0.0);
    return s;
}

// Everything that can be refused without a HIP call, in the order the header gives. (pt_fail takes a NULL context.)
static int pt_ao_check(pt_context* c, const pt_ao_params* p, const double* positions, const double* normals, const pt_ao_buffers* out) {
    if (!c || !p || !positions || !normals || !out) return pt_fail(c, PT_ERR_ARGUMENT, "pt_ao: NULL context, params, positions, normals or buffers");
    if (!(out->occluded || out->valid || out->bent)) return pt_fail(c, PT_ERR_ARGUMENT, "pt_ao: no output buffer asked for");
    if (const char* why = pt_ao_params_error(p)) return pt_fail(c, PT_ERR_ARGUMENT, why);
    if (!c->have_scene) return pt_fail(c, PT_ERR_NO_SCENE, "no scene uploaded");
    // (the ray queries' words, whichever of the three kinds is open: the pass object is theirs, and pt_rays_finish closes all of them)
    if (c->rays.pass.pending) return pt_fail(c, PT_ERR_ARGUMENT, "a pt_rays_device / pt_segments_device pass is in flight: pt_rays_finish first");
    return PT_OK;
}

// The work layout of a launch: PORTRAYER_AO_LAYOUT=point|sample, else the one that measured faster.
static int pt_ao_layout() {
    if (const char* e = getenv("PORTRAYER_AO_LAYOUT")) {
        if (!strcmp(e, "point")) return PT_AO_POINT_MAJOR;
        if (!strcmp(e, "sample")) return PT_AO_SAMPLE_MAJOR;
    }
    return PT_AO_POINT_MAJOR;
}

// Queues the pass on `stream` (pt_pass_open ... pt_pass_seal), as pt_rays_common does and on its PtPass. Every pointer is a DEVICE pointer; n > 0. The LDS stack
// area is sized as for the ray queries, less the point-major layout's column of directions.
static int pt_ao_common(pt_context* c, const pt_ao_params* p, const double* d_positions, const double* d_normals, const pt_ao_buffers& out, hipStream_t stream) {
    PtPass& v = c->rays.pass;
    int rc = pt_pass_prepare(c, v);
    if (rc) return rc;
    const int layout = pt_ao_layout();
    PtAoArgs a;
    memset(&a, 0, sizeof a);
    a.r.scene = c->view;
    a.n = p->n; a.positions = d_positions; a.normals = d_normals;
    a.set = pt_ao_set(p);
    a.samples = p->samples;
    while ((1u << a.log2_samples) < p->samples) a.log2_samples++;
    a.radius = p->radius;
    a.occluded = out.occluded; a.valid = out.valid; a.bent = out.bent;
    const uint64_t per_item = layout == PT_AO_POINT_MAJOR ? 64u >> a.log2_samples : 64u;  // points of a wavefront
    a.r.n_items = (uint32_t)((p->n + per_item - 1) / per_item);                          // (n <= PT_AO_MAX = 2^24: at most 2^24 items)
    a.r.stack_lds_cap = pt_stack_lds_cap(a.r.scene, pt_block_budget(pt_ao_waves(a.r.scene.mode)), pt_ao_frame_bytes(layout));  // (as pt_walk_sizing)
    a.r.grid_share = 1;
    uint32_t grid = 0;
    PT_HIP(c, pt_ao_dispatch(a, layout, c->n_cu, stream, &grid, false));
    if ((rc = pt_pass_open(c, v, a.r, grid, false, stream))) return rc;
    PT_HIP(c, pt_ao_dispatch(a, layout, c->n_cu, stream, &grid, true));
    return pt_pass_seal(c, v);
}

extern "C" int pt_ao(pt_context* c, const pt_ao_params* p, const double* positions, const double* normals, const pt_ao_buffers* host_out, double* kernel_ms) {
    int rc = pt_ao_check(c, p, positions, normals, host_out);
    if (rc) return rc;
    if (kernel_ms) *kernel_ms = 0.0;
    if (p->n == 0) return PT_OK;
    PT_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)p->n;
    // the ray-query pass's device copies: positions and normals where it keeps origins and directions, the results in three of its output buffers
    pt_context::Rays& v = c->rays;
    PtStage s[5] = {pt_stage_input(positions, v.in[0], n * 24), pt_stage_input(normals, v.in[1], n * 24),
                    pt_stage_output(host_out->occluded, v.out[3], n * 4), pt_stage_output(host_out->valid, v.out[6], n), pt_stage_output(host_out->bent, v.out[1], n * 24)};
    if ((rc = pt_stage_in(c, s))) return rc;
    const pt_ao_buffers d_out = {(uint32_t*)s[2].dev, (uint8_t*)s[3].dev, (double*)s[4].dev};
    return pt_stage_out(c, v.pass, pt_ao_common(c, p, (const double*)s[0].dev, (const double*)s[1].dev, d_out, nullptr), s, kernel_ms);
}

extern "C" int pt_ao_device(pt_context* c, const pt_ao_params* p, const double* d_positions, const double* d_normals, const pt_ao_buffers* device_out, void* hip_stream) {
    int rc = pt_ao_check(c, p, d_positions, d_normals, device_out);
    if (rc) return rc;
    if (p->n == 0) return PT_OK;  // nothing queued, nothing to finish
    PT_HIP(c, hipSetDevice(c->device));
    return pt_pass_device_tail(c, c->rays.pass, pt_ao_common(c, p, d_positions, d_normals, *device_out, (hipStream_t)hip_stream));
}

// The pass is the ray queries': one function closes any of them.
extern "C" int pt_ao_finish(pt_context* c, double* kernel_ms) { return pt_rays_finish(c, kernel_ms); }

// Steps 1 to 8 of the contract on the host: pt_ao_valid and pt_ao_ray as this translation unit's host pass compiles them (-ffp-contract=off).
extern "C" int pt_test_ao_rays_host(uint64_t n, const pt_ao_params* p, const double* positions, const double* normals, double* origins, double* directions, uint8_t* valid) {
    if (!p || !positions || !normals || !origins || !directions || !valid) return PT_ERR_ARGUMENT;
    if (pt_ao_params_error(p)) return PT_ERR_ARGUMENT;
    const PtAoSet set = pt_ao_set(p);
    for (uint64_t i = 0; i < n; i++) {
        const PtVec3 P = pt_v3(positions[3 * i], positions[3 * i + 1], positions[3 * i + 2]), N = pt_v3(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]);
        valid[i] = pt_ao_valid(P, N) ? 1 : 0;
        for (uint32_t k = 0; k < p->samples; k++) {
            PtVec3 o = pt_v3(0.0, 0.0, 0.0), d = o;
            if (valid[i]) pt_ao_ray(set, P, N, p->first_index + i, k, &o, &d);
            double* oo = origins + 3 * (i * p->samples + k);
            double* dd = directions + 3 * (i * p->samples + k);
            oo[0] = o.x; oo[1] = o.y; oo[2] = o.z;
            dd[0] = d.x; dd[1] = d.y; dd[2] = d.z;
        }
    }
    return PT_OK;
}

extern "C" int pt_test_ao_tables(double* dirs, double* rot) {
    if (!dirs || !rot) return PT_ERR_ARGUMENT;
    memcpy(dirs, PT_AO_DIRS, sizeof PT_AO_DIRS);
    memcpy(rot, PT_AO_ROT, sizeof PT_AO_ROT);
    return PT_OK;
}

// ------------------------------------------------------------------------------------------------
// Direct light (pt_direct.h: the contract; pt_direct_inst.hip: the kernel): a ray-query pass, on that pass's PtPass, as pt_ao is
// ------------------------------------------------------------------------------------------------
static hipError_t pt_direct_dispatch(const PtDirectArgs& a, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    PT_MODE_LAUNCH(pt_direct_launch_mode_, a.r.scene.mode, a, n_cu, stream, grid, launch)
}

// What pt_direct refuses of a parameter block, in the order the header gives; null: nothing. (Also pt_test_direct_host's check.)
static const char* pt_direct_params_error(const pt_direct_params* p) {
    if (p->n > PT_AO_MAX) return "pt_direct: more than PT_AO_MAX points in one call";
    if (p->samples == 0 || p->samples > 64 || (p->samples & (p->samples - 1)) != 0) return "pt_direct: samples must be a power of two, 1 .. 64";
    if (!std::isfinite(p->bias) || p->bias < 0.0) return "pt_direct: bias must be finite and not negative";
    if (p->flags & ~(PT_AO_FACE_EYE | PT_DIRECT_TO_LIGHT)) return "pt_direct: unknown flags";
    if ((p->flags & PT_AO_FACE_EYE) && !(std::isfinite(p->eye[0]) && std::isfinite(p->eye[1]) && std::isfinite(p->eye[2]))) return "pt_direct: PT_AO_FACE_EYE needs a finite eye";
    return nullptr;
}

static_assert(PT_DIRECT_FLAG_FACE_EYE == PT_AO_FACE_EYE && PT_DIRECT_FLAG_TO_LIGHT == PT_DIRECT_TO_LIGHT, "pt_direct.h restates the header's flags");

static PtDirectSet pt_direct_set(const pt_direct_params* p) {
    PtDirectSet s;
    s.seed = p->seed; s.first_index = p->first_index; s.pass = p->pass; s.flags = p->flags; s.samples = p->samples; s.bias = p->bias;
    s.eye = (p->flags & PT_AO_FACE_EYE) ? pt_v3(p->eye[0], p->eye[1], p->eye[2]) : pt_v3(0.0, 0.0, 0.0);
    return s;
}

// Everything that can be refused without a HIP call, in the order the header gives. (pt_fail takes a NULL context.)
static int pt_direct_check(pt_context* c, const pt_direct_params* p, const double* positions, const double* normals, const pt_direct_buffers* out) {
    if (!c || !p || !positions || !normals || !out) return pt_fail(c, PT_ERR_ARGUMENT, "pt_direct: NULL context, params, positions, normals or buffers");
    if (!(out->sum || out->lit || out->valid)) return pt_fail(c, PT_ERR_ARGUMENT, "pt_direct: no output buffer asked for");
    if (const char* why = pt_direct_params_error(p)) return pt_fail(c, PT_ERR_ARGUMENT, why);
    if (!c->have_scene) return pt_fail(c, PT_ERR_NO_SCENE, "no scene uploaded");
    // (the ray queries' words, whichever of the four kinds is open: the pass object is theirs, and pt_rays_finish closes all of them)
    if (c->rays.pass.pending) return pt_fail(c, PT_ERR_ARGUMENT, "a pt_rays_device / pt_segments_device pass is in flight: pt_rays_finish first");
    return PT_OK;
}

// Queues the pass on `stream` (pt_pass_open ... pt_pass_seal), as pt_ao_common does and on its PtPass. Every pointer is a DEVICE pointer; n > 0. The LDS stack
// area is sized as for the ray queries, less the wavefronts' columns of terms and sums.
static int pt_direct_common(pt_context* c, const pt_direct_params* p, const double* d_positions, const double* d_normals, const pt_direct_buffers& out, hipStream_t stream) {
    PtPass& v = c->rays.pass;
    int rc = pt_pass_prepare(c, v);
    if (rc) return rc;
    PtDirectArgs a;
    memset(&a, 0, sizeof a);
    a.r.scene = c->view;
    a.n = p->n; a.positions = d_positions; a.normals = d_normals;
    a.set = pt_direct_set(p);
    a.sum = out.sum; a.lit = out.lit; a.valid = out.valid;
    a.r.n_items = (uint32_t)((p->n + 63u) / 64u);  // (n <= PT_AO_MAX = 2^24)
    a.r.stack_lds_cap = pt_stack_lds_cap(a.r.scene, pt_block_budget(pt_direct_waves(a.r.scene.mode)), pt_direct_frame_bytes());  // (as pt_walk_sizing)
    a.r.grid_share = 1;
    uint32_t grid = 0;
    PT_HIP(c, pt_direct_dispatch(a, c->n_cu, stream, &grid, false));
    if ((rc = pt_pass_open(c, v, a.r, grid, false, stream))) return rc;
    PT_HIP(c, pt_direct_dispatch(a, c->n_cu, stream, &grid, true));
    return pt_pass_seal(c, v);
}

extern "C" int pt_direct(pt_context* c, const pt_direct_params* p, const double* positions, const double* normals, const pt_direct_buffers* host_out, double* kernel_ms) {
    int rc = pt_direct_check(c, p, positions, normals, host_out);
    if (rc) return rc;
    if (kernel_ms) *kernel_ms = 0.0;
    if (p->n == 0) return PT_OK;
    PT_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)p->n;
    // the ray-query pass's device copies: positions and normals where it keeps origins and directions, the results in three of its output buffers
    pt_context::Rays& v = c->rays;
    PtStage s[5] = {pt_stage_input(positions, v.in[0], n * 24), pt_stage_input(normals, v.in[1], n * 24),
                    pt_stage_output(host_out->sum, v.out[1], n * 24), pt_stage_output(host_out->lit, v.out[3], n * 4), pt_stage_output(host_out->valid, v.out[6], n)};
    if ((rc = pt_stage_in(c, s))) return rc;
    const pt_direct_buffers d_out = {(double*)s[2].dev, (uint32_t*)s[3].dev, (uint8_t*)s[4].dev};
    return pt_stage_out(c, v.pass, pt_direct_common(c, p, (const double*)s[0].dev, (const double*)s[1].dev, d_out, nullptr), s, kernel_ms);
}

extern "C" int pt_direct_device(pt_context* c, const pt_direct_params* p, const double* d_positions, const double* d_normals, const pt_direct_buffers* device_out, void* hip_stream) {
    int rc = pt_direct_check(c, p, d_positions, d_normals, device_out);
    if (rc) return rc;
    if (p->n == 0) return PT_OK;  // nothing queued, nothing to finish
    PT_HIP(c, hipSetDevice(c->device));
    const uint64_t n = p->n;
    if ((rc = pt_check_device_pointer(c, d_positions, n * 24, "pt_direct_device: d_positions"))) return rc;
    if ((rc = pt_check_device_pointer(c, d_normals, n * 24, "pt_direct_device: d_normals"))) return rc;
    if (device_out->sum && (rc = pt_check_device_pointer(c, device_out->sum, n * 24, "pt_direct_device: sum"))) return rc;
    if (device_out->lit && (rc = pt_check_device_pointer(c, device_out->lit, n * 4, "pt_direct_device: lit"))) return rc;
    if (device_out->valid && (rc = pt_check_device_pointer(c, device_out->valid, n, "pt_direct_device: valid"))) return rc;
    return pt_pass_device_tail(c, c->rays.pass, pt_direct_common(c, p, d_positions, d_normals, *device_out, (hipStream_t)hip_stream));
}

// The pass is the ray queries': one function closes any of them.
extern "C" int pt_direct_finish(pt_context* c, double* kernel_ms) { return pt_rays_finish(c, kernel_ms); }

// Steps 1 to 7 and 9 of the contract on the host: pt_direct.h's functions as this translation unit's host pass compiles them (-ffp-contract=off).
extern "C" int pt_test_direct_host(uint64_t n, const pt_direct_params* p, const double* positions, const double* normals, uint32_t n_lights, const double* lights, double* origins,
                                   double* directions, double* t_max, double* terms, uint8_t* valid) {
    if (!p || !positions || !normals || (n_lights && !lights) || !origins || !directions || !t_max || !terms || !valid) return PT_ERR_ARGUMENT;
    if (pt_direct_params_error(p)) return PT_ERR_ARGUMENT;
    const PtDirectSet set = pt_direct_set(p);
    const uint64_t S = p->samples;
    for (uint64_t i = 0; i < n; i++) {
        const PtVec3 P = pt_v3(positions[3 * i], positions[3 * i + 1], positions[3 * i + 2]), N = pt_v3(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]);
        valid[i] = pt_direct_valid(P, N) ? 1 : 0;
        PtVec3 o = pt_v3(0.0, 0.0, 0.0), nrm = o;
        if (valid[i]) pt_direct_point(set, P, N, &o, &nrm);
        origins[3 * i] = o.x; origins[3 * i + 1] = o.y; origins[3 * i + 2] = o.z;
        uint32_t j = 0;
        for (uint32_t li = 0; li < n_lights; li++) {
            const double* light = lights + 15 * (size_t)li;
            for (uint32_t k = 0; k < p->samples; k++) {
                PtVec3 d = pt_v3(0.0, 0.0, 0.0), term = d;
                double tm = 0.0;
                if (valid[i]) pt_direct_sample(set, o, nrm, pt_direct_light_position(set, light, j, p->first_index + i, k), light, &d, &tm, &term);
                const uint64_t at = (i * n_lights + li) * S + k;
                directions[3 * at] = d.x; directions[3 * at + 1] = d.y; directions[3 * at + 2] = d.z;
                terms[3 * at] = term.x; terms[3 * at + 1] = term.y; terms[3 * at + 2] = term.z;
                t_max[at] = tm;
            }
            if (!pt_direct_is_point_light(light)) j++;
        }
    }
    return PT_OK;
}

// ------------------------------------------------------------------------------------------------
// Radiance along the caller's rays (pt_radiance.h)
// ------------------------------------------------------------------------------------------------
static hipError_t pt_radiance_dispatch(const PtRadianceArgs& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    PT_MODE_LAUNCH(pt_radiance_launch_mode_, a.r.scene.mode, a, tex, park, n_cu, stream, grid, launch)
}

// Everything that can be refused without a HIP call, in the order the header gives. (pt_fail takes a NULL context.)
static int pt_radiance_check(pt_context* c, const pt_radiance_params* p, const double* origins, const double* directions, const double* background, const double* rgb) {
    if (!c || !p || !origins || !directions || !background || !rgb) return pt_fail(c, PT_ERR_ARGUMENT, "pt_radiance: NULL context, params, origins, directions, background or rgb");
    if (p->n > PT_RAYS_MAX) return pt_fail(c, PT_ERR_ARGUMENT, "pt_radiance: more than PT_RAYS_MAX rays in one call");
    if ((p->reorder != 0 && p->reorder != 1) || (p->background_per_ray != 0 && p->background_per_ray != 1))
        return pt_fail(c, PT_ERR_ARGUMENT, "pt_radiance: reorder and background_per_ray are 0 or 1");
    if (!c->have_scene) return pt_fail(c, PT_ERR_NO_SCENE, "no scene uploaded");
    if (c->radiance.pass.pending) return pt_fail(c, PT_ERR_ARGUMENT, "a pt_radiance_device pass is in flight: pt_radiance_finish first");
    return PT_OK;
}

// Queues the pass on `stream` (pt_pass_open ... pt_pass_seal): between the pass's two events the keying and the sort (reorder = 1) and the shading kernel.
// Every pointer is a DEVICE pointer. LDS per block as a render's interpreter kernel has it (pt_interp_sizing).
static int pt_radiance_common(pt_context* c, const pt_radiance_params* p, const double* d_origins, const double* d_directions, const double* d_background, double* d_rgb, hipStream_t stream) {
    PtPass& v = c->radiance.pass;
    int rc = pt_pass_prepare(c, v);
    if (rc) return rc;
    PtRadianceArgs a;
    memset(&a, 0, sizeof a);  // (no occluder table, no counters, no work counter: null)
    a.r.scene = c->view;
    a.r.seed = p->seed;
    a.r.n_items = (uint32_t)((p->n + 63u) / 64u);  // (n <= PT_RAYS_MAX = 2^30)
    a.n = p->n; a.origins = d_origins; a.directions = d_directions; a.background = d_background; a.bg_stride = p->background_per_ray ? 3u : 0u;
    a.sample = p->sample; a.stream_base = p->stream_base; a.rgb = d_rgb;
    const PtInterp k = pt_interp_sizing(c, a.r);
    uint32_t grid = 0;
    PT_HIP(c, pt_radiance_dispatch(a, k.tex, k.park, c->n_cu, stream, &grid, false));
    if (p->reorder && (rc = pt_ray_sort_reserve(c, c->radiance.sort, p->n, &a.perm))) return rc;
    if ((rc = pt_pass_open(c, v, a.r, grid, true, stream))) return rc;
    if (p->reorder && (rc = pt_ray_sort_queue(c, c->radiance.sort, p->n, d_origins, d_directions, stream))) return rc;
    PT_HIP(c, pt_radiance_dispatch(a, k.tex, k.park, c->n_cu, stream, &grid, true));
    return pt_pass_seal(c, v);
}

extern "C" int pt_radiance(pt_context* c, const pt_radiance_params* p, const double* origins, const double* directions, const double* background, double* rgb, double* kernel_ms) {
    int rc = pt_radiance_check(c, p, origins, directions, background, rgb);
    if (rc) return rc;
    if (kernel_ms) *kernel_ms = 0.0;
    if (p->n == 0) return PT_OK;
    PT_HIP(c, hipSetDevice(c->device));
    pt_context::Radiance& v = c->radiance;
    const size_t n = (size_t)p->n, bg_bytes = p->background_per_ray ? n * 24 : 24;
    PtStage s[4] = {pt_stage_input(origins, v.in[0], n * 24), pt_stage_input(directions, v.in[1], n * 24), pt_stage_input(background, v.in[2], bg_bytes),
                    pt_stage_output(rgb, v.out, n * 24)};
    if ((rc = pt_stage_in(c, s))) return rc;
    rc = pt_radiance_common(c, p, (const double*)s[0].dev, (const double*)s[1].dev, (const double*)s[2].dev, (double*)s[3].dev, nullptr);
    return pt_stage_out(c, v.pass, rc, s, kernel_ms);
}

extern "C" int pt_radiance_device(pt_context* c, const pt_radiance_params* p, const double* d_origins, const double* d_directions, const double* d_background, double* d_rgb, void* hip_stream) {
    int rc = pt_radiance_check(c, p, d_origins, d_directions, d_background, d_rgb);
    if (rc) return rc;
    if (p->n == 0) return PT_OK;  // nothing queued, nothing to finish
    PT_HIP(c, hipSetDevice(c->device));
    return pt_pass_device_tail(c, c->radiance.pass, pt_radiance_common(c, p, d_origins, d_directions, d_background, d_rgb, (hipStream_t)hip_stream));
}

extern "C" int pt_radiance_finish(pt_context* c, double* kernel_ms) {
    if (!c) return PT_ERR_ARGUMENT;
    const int rc = pt_pass_finish(c, c->radiance.pass, "no pt_radiance_device pass in flight", kernel_ms);
    if (!c->radiance.pass.pending) c->film_open = nullptr;  // (a film's pass is closed here too)
    return rc;
}

// ------------------------------------------------------------------------------------------------
// Gather (pt_gather.h): the ambient-occlusion contract's rays, shaded and summed per point; a radiance pass for bookkeeping, on that pass's PtPass
// ------------------------------------------------------------------------------------------------
static hipError_t pt_gather_dispatch(const PtGatherArgs& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    PT_MODE_LAUNCH(pt_gather_launch_mode_, a.r.scene.mode, a, tex, park, n_cu, stream, grid, launch)
}

// Everything that can be refused without a HIP call, in the order the header gives. (pt_fail takes a NULL context.)
static int pt_gather_check(pt_context* c, const pt_gather_params* p, const double* positions, const double* normals, const double* background, const pt_gather_buffers* out) {
    if (!c || !p || !positions || !normals || !background || !out)
        return pt_fail(c, PT_ERR_ARGUMENT, "pt_gather: NULL context, params, positions, normals, background or buffers");
    if (!(out->sum || out->valid)) return pt_fail(c, PT_ERR_ARGUMENT, "pt_gather: no output buffer asked for");
    if (p->n > PT_AO_MAX) return pt_fail(c, PT_ERR_ARGUMENT, "pt_gather: more than PT_AO_MAX points in one call");
    if (p->samples == 0 || p->samples > 64 || (p->samples & (p->samples - 1)) != 0) return pt_fail(c, PT_ERR_ARGUMENT, "pt_gather: samples must be a power of two, 1 .. 64");
    if (!std::isfinite(p->bias) || p->bias < 0.0) return pt_fail(c, PT_ERR_ARGUMENT, "pt_gather: bias must be finite and not negative");
    if (p->flags & ~PT_AO_FACE_EYE) return pt_fail(c, PT_ERR_ARGUMENT, "pt_gather: unknown flags");
    if ((p->flags & PT_AO_FACE_EYE) && !(std::isfinite(p->eye[0]) && std::isfinite(p->eye[1]) && std::isfinite(p->eye[2])))
        return pt_fail(c, PT_ERR_ARGUMENT, "pt_gather: PT_AO_FACE_EYE needs a finite eye");
    if (!c->have_scene) return pt_fail(c, PT_ERR_NO_SCENE, "no scene uploaded");
    if (c->radiance.pass.pending) return pt_fail(c, PT_ERR_ARGUMENT, "a pt_radiance_device / pt_film_add_device / pt_gather_device pass is in flight: pt_radiance_finish first");
    return PT_OK;
}

// Queues the pass on `stream` (pt_pass_open ... pt_pass_seal) as pt_radiance_common does and on its PtPass. The point and result pointers are DEVICE pointers,
// `background` is the caller's HOST colour, copied into the argument block; n > 0. LDS per block as a render's interpreter kernel has it (pt_interp_sizing).
static int pt_gather_common(pt_context* c, const pt_gather_params* p, const double* d_positions, const double* d_normals, const double* background, const pt_gather_buffers& out,
                            hipStream_t stream) {
    PtPass& v = c->radiance.pass;
    int rc = pt_pass_prepare(c, v);
    if (rc) return rc;
    PtGatherArgs a;
    memset(&a, 0, sizeof a);  // (no occluder table, no counters, no work counter: null)
    a.r.scene = c->view;
    a.r.seed = p->seed;
    a.n = p->n; a.positions = d_positions; a.normals = d_normals;
    a.set = pt_ao_set(p);
    a.samples = p->samples;
    while ((1u << a.log2_samples) < p->samples) a.log2_samples++;
    for (int k = 0; k < 3; k++) a.background[k] = background[k];
    a.sum = out.sum; a.valid = out.valid;
    const uint64_t per_item = 64u >> a.log2_samples;              // points of a wavefront
    a.r.n_items = (uint32_t)((p->n + per_item - 1) / per_item);  // (n <= PT_AO_MAX = 2^24: at most 2^24 items)
    const PtInterp k = pt_interp_sizing(c, a.r);
    uint32_t grid = 0;
    PT_HIP(c, pt_gather_dispatch(a, k.tex, k.park, c->n_cu, stream, &grid, false));
    if ((rc = pt_pass_open(c, v, a.r, grid, true, stream))) return rc;
    PT_HIP(c, pt_gather_dispatch(a, k.tex, k.park, c->n_cu, stream, &grid, true));
    return pt_pass_seal(c, v);
}

extern "C" int pt_gather(pt_context* c, const pt_gather_params* p, const double* positions, const double* normals, const double* background, const pt_gather_buffers* host_out,
                         double* kernel_ms) {
    int rc = pt_gather_check(c, p, positions, normals, background, host_out);
    if (rc) return rc;
    if (kernel_ms) *kernel_ms = 0.0;
    if (p->n == 0) return PT_OK;
    PT_HIP(c, hipSetDevice(c->device));
    pt_context::Radiance& v = c->radiance;
    const size_t n = (size_t)p->n;
    // the radiance pass's device copies: positions and normals where it keeps origins and directions, the sums in its output, the flags where its background goes
    PtStage s[4] = {pt_stage_input(positions, v.in[0], n * 24), pt_stage_input(normals, v.in[1], n * 24),
                    pt_stage_output(host_out->sum, v.out, n * 24), pt_stage_output(host_out->valid, v.in[2], n)};
    if ((rc = pt_stage_in(c, s))) return rc;
    const pt_gather_buffers d_out = {(double*)s[2].dev, (uint8_t*)s[3].dev};
    return pt_stage_out(c, v.pass, pt_gather_common(c, p, (const double*)s[0].dev, (const double*)s[1].dev, background, d_out, nullptr), s, kernel_ms);
}

extern "C" int pt_gather_device(pt_context* c, const pt_gather_params* p, const double* d_positions, const double* d_normals, const double* background,
                                const pt_gather_buffers* device_out, void* hip_stream) {
    int rc = pt_gather_check(c, p, d_positions, d_normals, background, device_out);
    if (rc) return rc;
    if (p->n == 0) return PT_OK;  // nothing queued, nothing to finish
    PT_HIP(c, hipSetDevice(c->device));
    return pt_pass_device_tail(c, c->radiance.pass, pt_gather_common(c, p, d_positions, d_normals, background, *device_out, (hipStream_t)hip_stream));
}

// The pass is the radiance pass's: one function closes either.
extern "C" int pt_gather_finish(pt_context* c, double* kernel_ms) { return pt_radiance_finish(c, kernel_ms); }

// ------------------------------------------------------------------------------------------------
// Probe (pt_probe_inst.hip, pt_probe.hip): the probe contract's rays (pt_probe.h) over a point's whole sphere, shaded, weighted with the order-2 spherical-harmonic
// basis and summed per probe; a radiance pass for bookkeeping, on that pass's PtPass
// ------------------------------------------------------------------------------------------------
static hipError_t pt_probe_dispatch(const PtProbeArgs& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    PT_MODE_LAUNCH(pt_probe_launch_mode_, a.r.scene.mode, a, tex, park, n_cu, stream, grid, launch)
}

static bool pt_probe_samples_ok(uint32_t s) { return s == 64 || s == 128 || s == 256 || s == 512 || s == 1024; }

// Everything that can be refused without a HIP call, in the order the header gives. (pt_fail takes a NULL context.)
static int pt_probe_check(pt_context* c, const pt_probe_params* p, const double* positions, const double* background, const pt_probe_buffers* out) {
    if (!c || !p || !positions || !background || !out) return pt_fail(c, PT_ERR_ARGUMENT, "pt_probe: NULL context, params, positions, background or buffers");
    if (!(out->sh || out->valid)) return pt_fail(c, PT_ERR_ARGUMENT, "pt_probe: no output buffer asked for");
    if (p->n > PT_PROBE_MAX) return pt_fail(c, PT_ERR_ARGUMENT, "pt_probe: more than PT_PROBE_MAX probes in one call");
    if (!pt_probe_samples_ok(p->samples)) return pt_fail(c, PT_ERR_ARGUMENT, "pt_probe: samples must be 64, 128, 256, 512 or 1024");
    if (!c->have_scene) return pt_fail(c, PT_ERR_NO_SCENE, "no scene uploaded");
    if (c->radiance.pass.pending)
        return pt_fail(c, PT_ERR_ARGUMENT, "a pt_radiance_device / pt_film_add_device / pt_gather_device / pt_probe_device pass is in flight: pt_radiance_finish first");
    return PT_OK;
}

// The most the pass keeps of partial sums - 216 bytes per (probe, round of 64 samples) - between its kernel and its fold: a call with more runs as several
// launches. PORTRAYER_PROBE_SCRATCH=<bytes> lowers the bound (tests: a handful of probes across several launches); never below one probe's partials.
#define PT_PROBE_SCRATCH_BYTES ((size_t)32 << 20)
static size_t pt_probe_scratch_bound() {
    size_t bound = PT_PROBE_SCRATCH_BYTES;
    if (const char* e = getenv("PORTRAYER_PROBE_SCRATCH")) { const long long b = atoll(e); if (b > 0 && (unsigned long long)b < bound) bound = (size_t)b; }
    return bound;
}

// Queues the pass on `stream` (pt_pass_open ... pt_pass_seal) as pt_gather_common does and on its PtPass. The position and result pointers are DEVICE pointers,
// `background` is the caller's HOST colour, copied into the argument block; n > 0. S = 64: one launch, the kernel stores `sh`. S = 64 R, R > 1, with `sh` wanted:
// per at most `chunk` probes the kernel and the fold of its partials (the queues zeroed again in between; the overflow flag stays: pt_film_add_common) - a
// launch is a call of its own with first_index moved on, which the contract makes invisible.
static int pt_probe_common(pt_context* c, const pt_probe_params* p, const double* d_positions, const double* background, const pt_probe_buffers& out, hipStream_t stream) {
    PtPass& v = c->radiance.pass;
    int rc = pt_pass_prepare(c, v);
    if (rc) return rc;
    PtProbeArgs a;
    memset(&a, 0, sizeof a);  // (no occluder table, no counters, no work counter: null)
    a.r.scene = c->view;
    a.r.seed = p->seed;
    a.set.seed = p->seed; a.set.pass = p->pass;
    a.samples = p->samples;
    while ((64u << a.log2_rounds) < p->samples) a.log2_rounds++;
    const uint32_t rounds = 1u << a.log2_rounds;
    for (int k = 0; k < 3; k++) a.background[k] = background[k];
    const bool fold = rounds > 1 && out.sh;
    uint64_t chunk = p->n;
    if (fold) {
        const size_t per_probe = (size_t)rounds * PT_PROBE_VALUES * sizeof(double);
        chunk = std::min<uint64_t>(p->n, std::max<size_t>(1, pt_probe_scratch_bound() / per_probe));
        if ((rc = pt_reserve(c, c->radiance.probe_partial, (size_t)chunk * per_probe))) return rc;
    }
    // the buffers are sized for the call's largest launch (its first); the later ones use a prefix of the same lanes
    auto set_launch = [&](uint64_t first, uint64_t m) {
        a.n = m;
        a.positions = d_positions + 3 * first;
        a.set.first_index = p->first_index + first;  // (modulo 2^64, as the stream index is)
        a.sh = !fold && out.sh ? out.sh + PT_PROBE_VALUES * first : nullptr;
        a.partial = fold ? (double*)c->radiance.probe_partial.p : nullptr;
        a.valid = out.valid ? out.valid + first : nullptr;
        a.r.n_items = (uint32_t)(m << a.log2_rounds);  // (n <= PT_PROBE_MAX = 2^20, R <= 16: at most 2^24 items)
    };
    set_launch(0, chunk);
    const PtInterp k = pt_interp_sizing(c, a.r);
    uint32_t grid = 0;
    PT_HIP(c, pt_probe_dispatch(a, k.tex, k.park, c->n_cu, stream, &grid, false));
    if ((rc = pt_pass_open(c, v, a.r, grid, true, stream))) return rc;
    for (uint64_t first = 0; first < p->n; first += chunk) {
        const uint64_t m = std::min<uint64_t>(chunk, p->n - first);
        set_launch(first, m);
        if (first) PT_HIP(c, hipMemsetAsync((char*)v.misc.p + 256, 0, PT_PASS_MISC_BYTES - 256, stream));  // the queues again; the overflow flag stays
        uint32_t g = 0;
        PT_HIP(c, pt_probe_dispatch(a, k.tex, k.park, c->n_cu, stream, &g, true));  // (g <= grid: no more items than the launch the buffers were sized for)
        if (fold) PT_HIP(c, pt_probe_fold_launch(a.partial, out.sh + PT_PROBE_VALUES * first, m, rounds, stream));
    }
    return pt_pass_seal(c, v);
}

extern "C" int pt_probe(pt_context* c, const pt_probe_params* p, const double* positions, const double* background, const pt_probe_buffers* host_out, double* kernel_ms) {
    int rc = pt_probe_check(c, p, positions, background, host_out);
    if (rc) return rc;
    if (kernel_ms) *kernel_ms = 0.0;
    if (p->n == 0) return PT_OK;
    PT_HIP(c, hipSetDevice(c->device));
    pt_context::Radiance& v = c->radiance;
    const size_t n = (size_t)p->n, sh_bytes = n * PT_PROBE_VALUES * sizeof(double);
    // the radiance pass's device copies: positions where it keeps origins, the sums in its output, the flags where its background goes
    PtStage s[3] = {pt_stage_input(positions, v.in[0], n * 24), pt_stage_output(host_out->sh, v.out, sh_bytes), pt_stage_output(host_out->valid, v.in[2], n)};
    if ((rc = pt_stage_in(c, s))) return rc;
    const pt_probe_buffers d_out = {(double*)s[1].dev, (uint8_t*)s[2].dev};
    return pt_stage_out(c, v.pass, pt_probe_common(c, p, (const double*)s[0].dev, background, d_out, nullptr), s, kernel_ms);
}

extern "C" int pt_probe_device(pt_context* c, const pt_probe_params* p, const double* d_positions, const double* background, const pt_probe_buffers* device_out,
                               void* hip_stream) {
    int rc = pt_probe_check(c, p, d_positions, background, device_out);
    if (rc) return rc;
    if (p->n == 0) return PT_OK;  // nothing queued, nothing to finish
    PT_HIP(c, hipSetDevice(c->device));
    return pt_pass_device_tail(c, c->radiance.pass, pt_probe_common(c, p, d_positions, background, *device_out, (hipStream_t)hip_stream));
}

// The pass is the radiance pass's: one function closes either.
extern "C" int pt_probe_finish(pt_context* c, double* kernel_ms) { return pt_radiance_finish(c, kernel_ms); }

// Steps 1 to 5 of the contract on the host: pt_probe_valid, pt_probe_dir and pt_probe_basis as this translation unit's host pass compiles them
// (-ffp-contract=off). Zeros for an invalid probe.
extern "C" int pt_test_probe_host(uint64_t n, const pt_probe_params* p, const double* positions, double* origins, double* directions, double* basis, uint8_t* valid) {
    if (!p || !positions || !origins || !directions || !basis || !valid) return PT_ERR_ARGUMENT;
    if (!pt_probe_samples_ok(p->samples)) return PT_ERR_ARGUMENT;
    PtProbeSet set;
    set.seed = p->seed; set.first_index = p->first_index; set.pass = p->pass;
    for (uint64_t i = 0; i < n; i++) {
        const PtVec3 P = pt_v3(positions[3 * i], positions[3 * i + 1], positions[3 * i + 2]);
        valid[i] = pt_probe_valid(P) ? 1 : 0;
        for (uint32_t k = 0; k < p->samples; k++) {
            PtVec3 o = pt_v3(0.0, 0.0, 0.0), d = o;
            double Y[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (valid[i]) { o = P; d = pt_probe_dir(set, p->first_index + i, k); pt_probe_basis(d, Y); }
            double* oo = origins + 3 * (i * p->samples + k);
            double* dd = directions + 3 * (i * p->samples + k);
            oo[0] = o.x; oo[1] = o.y; oo[2] = o.z;
            dd[0] = d.x; dd[1] = d.y; dd[2] = d.z;
            memcpy(basis + 9 * (i * p->samples + k), Y, sizeof Y);
        }
    }
    return PT_OK;
}

extern "C" int pt_test_probe_tables(double* dirs, double* sh) {
    if (!dirs || !sh) return PT_ERR_ARGUMENT;
    memcpy(dirs, PT_PROBE_DIRS, sizeof PT_PROBE_DIRS);
    memcpy(sh, PT_PROBE_SH, sizeof PT_PROBE_SH);
    return PT_OK;
}

// ------------------------------------------------------------------------------------------------
// Film: samples accumulate on the device (pt_film.h, pt_film.hip)
// ------------------------------------------------------------------------------------------------
static hipError_t pt_film_dispatch(const PtFilmArgs& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    PT_MODE_LAUNCH(pt_film_launch_mode_, a.r.scene.mode, a, tex, park, n_cu, stream, grid, launch)
}

static hipError_t pt_lens_dispatch(const PtLensArgs& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    PT_MODE_LAUNCH(pt_lens_launch_mode_, a.f.r.scene.mode, a, tex, park, n_cu, stream, grid, launch)
}

#define PT_FILM_COUNT_MAX 0x80000000u  // a pixel holds at most 2^31 samples: count + a launch's lane offset never wraps

// The context's own film, and no pass of its own in flight (`busy`: calls that read or write its state from the host). The handle is looked up, not
// dereferenced: a film of another context, or one already destroyed, is refused like a NULL.
static int pt_film_handle(pt_context* c, pt_film* f, bool busy, const char* who) {
    if (!c) return PT_ERR_ARGUMENT;
    if (!f || std::find(c->films.begin(), c->films.end(), f) == c->films.end()) return pt_fail(c, PT_ERR_ARGUMENT, std::string(who) + ": NULL film, or not a film of this context");
    if (busy && c->radiance.pass.pending && c->film_open == f) return pt_fail(c, PT_ERR_ARGUMENT, std::string(who) + ": a pt_film_add_device pass of this film is in flight: pt_radiance_finish first");
    return PT_OK;
}

static int pt_film_create_common(pt_context* c, uint32_t width, uint32_t height, pt_film** out, bool moments) {
    if (out) *out = nullptr;
    if (!c || !out) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_create: NULL context or out");
    if (width == 0 || height == 0 || (uint64_t)width * height >= 0x80000000ull) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_create: width and height must be positive, below 2^31 pixels");
    PT_HIP(c, hipSetDevice(c->device));
    pt_film* f = new pt_film();
    f->ctx = c; f->width = width; f->height = height;
    const size_t n = (size_t)width * height;
    int rc;
    f->moments = moments;
    if ((rc = pt_reserve(c, f->total, n * 24)) || (rc = pt_reserve(c, f->partial, n * 24)) || (rc = pt_reserve(c, f->count, n * 4)) || (moments && (rc = pt_reserve(c, f->q, n * 8)))) {
        delete f;
        return rc;
    }
    if ((moments && hipMemset(f->q.p, 0, n * 8) != hipSuccess) || hipMemset(f->total.p, 0, n * 24) != hipSuccess || hipMemset(f->partial.p, 0, n * 24) != hipSuccess || hipMemset(f->count.p, 0, n * 4) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        delete f;
        return pt_fail(c, PT_ERR_DEVICE, "pt_film_create: clearing the film failed");
    }
    f->counts.assign(n, 0u);
    c->films.push_back(f);
    *out = f;
    return PT_OK;
}
extern "C" int pt_film_create(pt_context* c, uint32_t width, uint32_t height, pt_film** out) { return pt_film_create_common(c, width, height, out, false); }
extern "C" int pt_film_create_moments(pt_context* c, uint32_t width, uint32_t height, pt_film** out) { return pt_film_create_common(c, width, height, out, true); }

extern "C" int pt_film_destroy(pt_context* c, pt_film* f) {
    int rc = pt_film_handle(c, f, true, "pt_film_destroy");
    if (rc) return rc;
    PT_HIP(c, hipSetDevice(c->device));
    c->films.erase(std::find(c->films.begin(), c->films.end(), f));
    delete f;  // (hipFree waits for whatever still reads the buffers)
    return PT_OK;
}

// The counts to zero: total and partial need no clearing, the first sample of a pixel is assigned (pt_film_fold).
extern "C" int pt_film_reset(pt_context* c, pt_film* f) {
    int rc = pt_film_handle(c, f, true, "pt_film_reset");
    if (rc) return rc;
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipMemset(f->count.p, 0, f->counts.size() * 4));
    PT_HIP(c, hipDeviceSynchronize());
    std::fill(f->counts.begin(), f->counts.end(), 0u);
    return PT_OK;
}

// Everything that can be refused without a HIP call, in the order the header gives.
static int pt_film_add_check(pt_context* c, pt_film* f, const pt_camera* cam, const double* background, const pt_film_params* p) {
    if (!c || !f || !cam || !background || !p) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_add / pt_film_add_lens: NULL context, film, camera, background or params");
    int rc = pt_film_handle(c, f, false, "pt_film_add");
    if (rc) return rc;
    if (p->sample_mode != PT_SAMPLE_CENTRE && p->sample_mode != PT_SAMPLE_RNG) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_add: bad sample_mode");
    if (p->background_rows != 0 && p->background_rows != 1) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_add: background_rows is 0 or 1");
    if (p->samples == 0) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_add: samples must be positive");
    if (p->slice.x0 >= f->width || p->slice.x1 >= f->width || p->slice.y0 >= f->height || p->slice.y1 >= f->height)
        return pt_fail(c, PT_ERR_SLICE, "slice corner outside the image (render.rs:79-90)");
    if (!c->have_scene) return pt_fail(c, PT_ERR_NO_SCENE, "no scene uploaded");
    if (c->radiance.pass.pending) return pt_fail(c, PT_ERR_ARGUMENT, "a pt_radiance_device / pt_film_add_device pass is in flight: pt_radiance_finish first");
    if (p->samples > PT_FILM_COUNT_MAX) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_add: a pixel's count would pass 2^31");
    for (uint32_t y = p->slice.y0; y <= p->slice.y1 && p->slice.x0 <= p->slice.x1; y++) {
        const uint32_t* row = f->counts.data() + (size_t)y * f->width;
        for (uint32_t x = p->slice.x0; x <= p->slice.x1; x++)
            if (row[x] > PT_FILM_COUNT_MAX - p->samples) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_add: a pixel's count would pass 2^31");
    }
    return PT_OK;
}
static bool pt_film_slice_empty(const pt_film_params* p) { return p->slice.x1 < p->slice.x0 || p->slice.y1 < p->slice.y0; }  // render.rs:60-65: an inverted slice renders nothing

// Queues the add on `stream` as a radiance pass (its PtPass: pt_pass_open ... pt_pass_seal): between the pass's two events, per at most `lw` samples, the
// sampling kernel and its fold (the queues zeroed again in between; the overflow flag stays). d_background is a DEVICE pointer. LDS per block as the radiance
// pass has it. The argument block is shared with pt_film_add_map:
static int pt_film_pass_args(pt_context* c, pt_film* f, const pt_camera* cam, const double* d_background, const pt_rect& slice, uint64_t seed, int32_t sample_mode, int32_t background_rows, uint32_t lw,
                             PtFilmArgs& a, PtInterp& k) {
    int rc = pt_pass_prepare(c, c->radiance.pass);
    if (rc) return rc;
    pt_render_params rp;
    memset(&rp, 0, sizeof rp);
    rp.width = f->width; rp.height = f->height; rp.slice = slice;
    rp.samples = 1; rp.seed = seed; rp.sample_mode = sample_mode; rp.background_rows = background_rows; rp.tile_rank = 0; rp.tile_ranks = 1;
    memset(&a, 0, sizeof a);  // (no occluder table, no counters, no work counter: null)
    pt_fill_args(c, cam, &rp, &a.r);  // the camera, the slice and its pixel slots; the work items are the film's own (the callers')
    a.r.background = d_background;
    a.lw = lw;
    a.count = (const uint32_t*)f->count.p;
    k = pt_interp_sizing(c, a.r);
    return PT_OK;
}

// lens: NULL for pt_film_add's pinhole samples (pt_film_kernel); else the lens contract's (pt_lens_kernel, pt_lens_inst.hip), which takes the same block with
// the lens behind it. Nothing but the launcher differs.
static int pt_film_add_common(pt_context* c, pt_film* f, const pt_camera* cam, const double* d_background, const pt_film_params* p, const pt_lens* lens, hipStream_t stream) {
    PtPass& v = c->radiance.pass;
    uint32_t lw = PT_FILM_LW;
    if (const char* e = getenv("PORTRAYER_FILM_LW")) { const int w = atoi(e); if (w == 8 || w == 64) lw = (uint32_t)w; }  // measurements (profiles/film)
    if (f->moments) lw = PT_FILM_LW;  // (the fold that keeps q takes at most PT_FILM_LW samples per launch: pt_film_map_round)
    PtFilmArgs a;
    PtInterp k;
    int rc = pt_film_pass_args(c, f, cam, d_background, p->slice, p->seed, p->sample_mode, p->background_rows, lw, a, k);
    if (rc) return rc;
    const uint32_t tiles = a.r.n_slots / 64u;
    auto dispatch = [&](uint32_t* g, bool launch) {
        if (!lens) return pt_film_dispatch(a, k.tex, k.park, c->n_cu, stream, g, launch);
        PtLensArgs la;
        la.f = a;
        la.lens.model = lens->model; la.lens.aperture = lens->aperture; la.lens.focus = lens->focus; la.lens.extent = lens->extent;
        return pt_lens_dispatch(la, k.tex, k.park, c->n_cu, stream, g, launch);
    };
    // the buffers are sized for the add's largest launch (its first: min(samples, lw) samples per pixel); the later ones use a prefix of the same lanes
    auto set_launch = [&](uint32_t m) {
        a.launch_samples = m;
        for (a.k_log2 = 0; (1u << a.k_log2) < m; a.k_log2++) { }
        a.r.n_items = tiles << a.k_log2;  // (tiles < 2^25, K <= 64)
    };
    set_launch(std::min(p->samples, lw));
    uint32_t grid = 0;
    PT_HIP(c, dispatch(&grid, false));
    if ((rc = pt_reserve(c, f->staging, (size_t)a.r.n_slots * a.lw * 24))) return rc;
    a.staging = (double*)f->staging.p;
    if ((rc = pt_pass_open(c, v, a.r, grid, true, stream))) return rc;
    for (uint32_t left = p->samples, first = 1; left > 0; first = 0) {
        const uint32_t m = std::min(left, lw);
        set_launch(m);
        if (!first) PT_HIP(c, hipMemsetAsync((char*)v.misc.p + 256, 0, PT_PASS_MISC_BYTES - 256, stream));  // the queues again; the overflow flag stays
        uint32_t g = 0;
        PT_HIP(c, dispatch(&g, true));  // (g <= grid: no more items than the launch the buffers were sized for)
        if (f->moments)  // the fold that keeps q as well: a uniform "map" of m, round 0 (pt_film_map.hip)
            PT_HIP(c, pt_film_fold_map_launch(a, nullptr, m, 0u, (double*)f->total.p, (double*)f->partial.p, (uint32_t*)f->count.p, (double*)f->q.p, stream));
        else
            PT_HIP(c, pt_film_fold_launch(a, (double*)f->total.p, (double*)f->partial.p, (uint32_t*)f->count.p, stream));
        left -= m;
    }
    if ((rc = pt_pass_seal(c, v))) return rc;
    for (uint32_t y = p->slice.y0; y <= p->slice.y1; y++) {  // the host's copy of the counts
        uint32_t* row = f->counts.data() + (size_t)y * f->width;
        for (uint32_t x = p->slice.x0; x <= p->slice.x1; x++) row[x] += p->samples;
    }
    return PT_OK;
}

// What pt_film_add_lens refuses beyond pt_film_add's list, in the header's order. No HIP call.
static int pt_lens_check(pt_context* c, const pt_lens* l) {
    if (!l) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_add_lens: NULL lens");
    if (l->model != PT_LENS_THIN && l->model != PT_LENS_ORTHO && l->model != PT_LENS_STEREO) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_add_lens: unknown lens model");
    if (l->model == PT_LENS_THIN) {
        if (!std::isfinite(l->aperture) || l->aperture < 0.0) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_add_lens: aperture must be finite and not negative");
        if (!std::isfinite(l->focus) || !(l->focus > 0.0)) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_add_lens: focus must be finite and positive");
    } else if (!std::isfinite(l->extent) || !(l->extent > 0.0)) {
        return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_add_lens: extent must be finite and positive");
    }
    return PT_OK;
}

// pt_film_add and pt_film_add_lens (lens_call: the check of `lens` stands behind pt_film_add's own refusals; lens == NULL otherwise)
static int pt_film_add_host(pt_context* c, pt_film* f, const pt_camera* cam, const pt_lens* lens, bool lens_call, const double* background, const pt_film_params* p, double* kernel_ms) {
    int rc = pt_film_add_check(c, f, cam, background, p);
    if (rc) return rc;
    if (lens_call && (rc = pt_lens_check(c, lens))) return rc;
    if (kernel_ms) *kernel_ms = 0.0;
    if (pt_film_slice_empty(p)) return PT_OK;
    PT_HIP(c, hipSetDevice(c->device));
    const size_t bg_bytes = (p->background_rows ? (size_t)f->height : (size_t)f->height * f->width) * 24;
    if ((rc = pt_reserve(c, f->bg, bg_bytes))) return rc;
    PT_HIP(c, hipMemcpy(f->bg.p, background, bg_bytes, hipMemcpyHostToDevice));
    if ((rc = pt_pass_settle(c, c->radiance.pass, pt_film_add_common(c, f, cam, (const double*)f->bg.p, p, lens, nullptr)))) return rc;
    return pt_pass_result(c, c->radiance.pass, kernel_ms);
}

static int pt_film_add_queued(pt_context* c, pt_film* f, const pt_camera* cam, const pt_lens* lens, bool lens_call, const double* d_background, const pt_film_params* p, void* hip_stream) {
    int rc = pt_film_add_check(c, f, cam, d_background, p);
    if (rc) return rc;
    if (lens_call && (rc = pt_lens_check(c, lens))) return rc;
    if (pt_film_slice_empty(p)) return PT_OK;  // nothing queued, nothing to finish
    PT_HIP(c, hipSetDevice(c->device));
    if ((rc = pt_pass_device_tail(c, c->radiance.pass, pt_film_add_common(c, f, cam, d_background, p, lens, (hipStream_t)hip_stream)))) return rc;
    c->film_open = f;
    return PT_OK;
}

extern "C" int pt_film_add(pt_context* c, pt_film* f, const pt_camera* cam, const double* background, const pt_film_params* p, double* kernel_ms) {
    return pt_film_add_host(c, f, cam, nullptr, false, background, p, kernel_ms);
}

extern "C" int pt_film_add_device(pt_context* c, pt_film* f, const pt_camera* cam, const double* d_background, const pt_film_params* p, void* hip_stream) {
    return pt_film_add_queued(c, f, cam, nullptr, false, d_background, p, hip_stream);
}

extern "C" int pt_film_add_lens(pt_context* c, pt_film* f, const pt_camera* cam, const pt_lens* lens, const double* background, const pt_film_params* p, double* kernel_ms) {
    return pt_film_add_host(c, f, cam, lens, true, background, p, kernel_ms);
}

extern "C" int pt_film_add_lens_device(pt_context* c, pt_film* f, const pt_camera* cam, const pt_lens* lens, const double* d_background, const pt_film_params* p, void* hip_stream) {
    return pt_film_add_queued(c, f, cam, lens, true, d_background, p, hip_stream);
}

// Steps 1 to 6 of the lens contract on the host: pt_lens_jitter and pt_lens_ray as this translation unit's host pass compiles them (-ffp-contract=off). The
// film's width gives the stream index y width + x; pixels outside width x height, a bad sample mode or a lens pt_film_add_lens refuses: PT_ERR_ARGUMENT.
extern "C" int pt_test_lens_rays_host(const pt_camera* cam, const pt_lens* lens, uint32_t width, uint32_t height, uint64_t seed, int32_t sample_mode, uint64_t n, const uint32_t* pixels_xy,
                                      const uint32_t* samples, double* origins, double* directions) {
    if (!cam || !lens || !pixels_xy || !samples || !origins || !directions) return PT_ERR_ARGUMENT;
    if (sample_mode != PT_SAMPLE_CENTRE && sample_mode != PT_SAMPLE_RNG) return PT_ERR_ARGUMENT;
    if (pt_lens_check(nullptr, lens)) return PT_ERR_ARGUMENT;
    PtCamera pc;
    for (int k = 0; k < 3; k++) pc.eye[k] = cam->eye[k];
    for (int k = 0; k < 12; k++) pc.view_to_world[k] = cam->view_to_world[k];
    pc.fov_factor = cam->fov_factor; pc.aspect = cam->aspect_ratio; pc.width = cam->width; pc.height = cam->height;  // (pt_fill_args)
    PtLensSet ls;
    ls.model = lens->model; ls.aperture = lens->aperture; ls.focus = lens->focus; ls.extent = lens->extent;
    for (uint64_t i = 0; i < n; i++)
        if (pixels_xy[2 * i] >= width || pixels_xy[2 * i + 1] >= height) return PT_ERR_ARGUMENT;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t x = pixels_xy[2 * i], y = pixels_xy[2 * i + 1], s = samples[i];
        const uint64_t pixel = (uint64_t)y * width + x;
        double jx, jy;
        pt_lens_jitter(seed, sample_mode == PT_SAMPLE_RNG, pixel, s, &jx, &jy);
        const PtRay r = pt_lens_ray(pc, ls, seed, pixel, s, (double)x + jx, (double)y + jy);
        origins[3 * i] = r.o.x; origins[3 * i + 1] = r.o.y; origins[3 * i + 2] = r.o.z;
        directions[3 * i] = r.d.x; directions[3 * i + 1] = r.d.y; directions[3 * i + 2] = r.d.z;
    }
    return PT_OK;
}

extern "C" int pt_film_resolve_device(pt_context* c, pt_film* f, void* d_rgb, double* d_linear, void* hip_stream) {
    if (!c || !f || (!d_rgb && !d_linear)) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_resolve_device: NULL context or film, or neither rgb nor linear");
    int rc = pt_film_handle(c, f, false, "pt_film_resolve_device");
    if (rc) return rc;
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, pt_film_resolve_launch(f->width, f->height, (const double*)f->total.p, (const double*)f->partial.p, (const uint32_t*)f->count.p, (uint8_t*)d_rgb, d_linear, (hipStream_t)hip_stream));
    return PT_OK;
}

extern "C" int pt_film_resolve(pt_context* c, pt_film* f, uint8_t* rgb, double* linear) {
    if (!c || !f || (!rgb && !linear)) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_resolve: NULL context or film, or neither rgb nor linear");
    int rc = pt_film_handle(c, f, true, "pt_film_resolve");
    if (rc) return rc;
    PT_HIP(c, hipSetDevice(c->device));
    const size_t n = f->counts.size();
    // pixels without samples keep the caller's bytes: where there are any, the caller's buffers go to the device first
    const bool holes = std::find(f->counts.begin(), f->counts.end(), 0u) != f->counts.end();
    if (rgb) {
        if ((rc = pt_reserve(c, f->out_rgb, n * 3))) return rc;
        if (holes) PT_HIP(c, hipMemcpy(f->out_rgb.p, rgb, n * 3, hipMemcpyHostToDevice));
    }
    if (linear) {
        if ((rc = pt_reserve(c, f->out_linear, n * 24))) return rc;
        if (holes) PT_HIP(c, hipMemcpy(f->out_linear.p, linear, n * 24, hipMemcpyHostToDevice));
    }
    PT_HIP(c, pt_film_resolve_launch(f->width, f->height, (const double*)f->total.p, (const double*)f->partial.p, (const uint32_t*)f->count.p, rgb ? (uint8_t*)f->out_rgb.p : nullptr,
                                     linear ? (double*)f->out_linear.p : nullptr, nullptr));
    if (rgb) PT_HIP(c, hipMemcpy(rgb, f->out_rgb.p, n * 3, hipMemcpyDeviceToHost));
    if (linear) PT_HIP(c, hipMemcpy(linear, f->out_linear.p, n * 24, hipMemcpyDeviceToHost));
    return PT_OK;
}

extern "C" int pt_film_counts(pt_context* c, pt_film* f, uint32_t* counts) {
    if (!c || !f || !counts) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_counts: NULL context, film or counts");
    int rc = pt_film_handle(c, f, true, "pt_film_counts");
    if (rc) return rc;
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipMemcpy(counts, f->count.p, f->counts.size() * 4, hipMemcpyDeviceToHost));  // the DEVICE's counts: what the kernels see
    std::copy(counts, counts + f->counts.size(), f->counts.begin());  // (behind a device map the host's copy was an upper bound: pt_film_add_map_device)
    return PT_OK;
}

// ------------------------------------------------------------------------------------------------
// Film, adaptive: a budget per pixel, a noise estimate, the budget of a refine pass (pt_film_map.h, pt_film_map.hip)
// ------------------------------------------------------------------------------------------------
static hipError_t pt_film_map_dispatch(const PtFilmMapArgs& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    PT_MODE_LAUNCH(pt_film_map_launch_mode_, a.f.r.scene.mode, a, tex, park, n_cu, stream, grid, launch)
}

static uint64_t pt_film_slice_slots(const pt_rect& s) { return (uint64_t)((s.x1 - s.x0 + 8u) / 8u) * ((s.y1 - s.y0 + 8u) / 8u) * 64u; }  // 8x8 tiles over the rectangle (pt_slot_to_pixel)

// Everything that can be refused without a HIP call. host_budget: the map where the host can read it (then a pixel's bound is its own m), else NULL.
// *most: the most any pixel of the slice gets (max_samples for a device map).
static int pt_film_add_map_check(pt_context* c, pt_film* f, const pt_camera* cam, const double* background, const pt_film_map_params* p, const uint32_t* budget, const uint32_t* host_budget,
                                 uint32_t* most) {
    if (!c || !f || !cam || !background || !p || !budget) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_add_map: NULL context, film, camera, background, params or budget");
    int rc = pt_film_handle(c, f, false, "pt_film_add_map");
    if (rc) return rc;
    if (p->sample_mode != PT_SAMPLE_CENTRE && p->sample_mode != PT_SAMPLE_RNG) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_add_map: bad sample_mode");
    if (p->background_rows != 0 && p->background_rows != 1) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_add_map: background_rows is 0 or 1");
    if (p->max_samples == 0 || p->max_samples > PT_FILM_MAP_MAX) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_add_map: max_samples is 1 .. PT_FILM_MAP_MAX");
    if (p->slice.x0 >= f->width || p->slice.x1 >= f->width || p->slice.y0 >= f->height || p->slice.y1 >= f->height)
        return pt_fail(c, PT_ERR_SLICE, "slice corner outside the image (render.rs:79-90)");
    if (!c->have_scene) return pt_fail(c, PT_ERR_NO_SCENE, "no scene uploaded");
    if (c->radiance.pass.pending) return pt_fail(c, PT_ERR_ARGUMENT, "a pt_radiance_device / pt_film_add_device pass is in flight: pt_radiance_finish first");
    *most = 0;
    if (p->slice.x1 < p->slice.x0 || p->slice.y1 < p->slice.y0) return PT_OK;
    if (pt_film_slice_slots(p->slice) >= PT_FILM_MAP_SLOTS_MAX) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_add_map: a slice of 2^29 pixel slots or more (an entry of the list is one u32)");
    for (uint32_t y = p->slice.y0; y <= p->slice.y1; y++) {
        const uint32_t* row = f->counts.data() + (size_t)y * f->width;
        const uint32_t* brow = host_budget ? host_budget + (size_t)y * f->width : nullptr;
        for (uint32_t x = p->slice.x0; x <= p->slice.x1; x++) {
            const uint32_t m = brow ? std::min(brow[x], p->max_samples) : p->max_samples;
            if (row[x] > PT_FILM_COUNT_MAX - m) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_add_map: a pixel's count would pass 2^31");
            *most = std::max(*most, m);
        }
    }
    return PT_OK;
}

// Queues the pass like pt_film_add_common; per launch round r < ceil(most / PT_FILM_LW): the plan (list + its length), the queues zeroed, the sampling kernel
// over the list, the fold. The grid and the buffers are sized from the host's upper bound of round 0: every slot taking min(most, PT_FILM_LW).
static int pt_film_add_map_common(pt_context* c, pt_film* f, const pt_camera* cam, const double* d_background, const pt_film_map_params* p, const uint32_t* d_budget, uint32_t most,
                                  hipStream_t stream) {
    PtPass& v = c->radiance.pass;
    PtFilmMapArgs a;
    memset(&a, 0, sizeof a);
    PtInterp k;
    int rc = pt_film_pass_args(c, f, cam, d_background, p->slice, p->seed, p->sample_mode, p->background_rows, PT_FILM_LW, a.f, k);
    if (rc) return rc;
    const uint32_t n_slots = a.f.r.n_slots;  // (< 2^29: n_slots * PT_FILM_LW fits a u32)
    auto bound = [&](uint32_t round) { return (uint32_t)(((uint64_t)n_slots * std::min<uint32_t>(most - round * PT_FILM_LW, PT_FILM_LW) + 63u) / 64u); };
    a.f.r.n_items = bound(0);
    a.f.launch_samples = PT_FILM_LW;
    uint32_t grid = 0;
    PT_HIP(c, pt_film_map_dispatch(a, k.tex, k.park, c->n_cu, stream, &grid, false));
    if ((rc = pt_reserve(c, f->list, 16 + (size_t)n_slots * PT_FILM_LW * 4)) || (rc = pt_reserve(c, f->plan_work, pt_film_plan_words(n_slots) * 4))) return rc;
    uint32_t* n_list = (uint32_t*)f->list.p;
    uint32_t* list = (uint32_t*)((char*)f->list.p + 16);
    a.list = list;
    a.n_list = n_list;
    if ((rc = pt_reserve(c, f->staging, (size_t)n_slots * PT_FILM_LW * 24))) return rc;
    a.f.staging = (double*)f->staging.p;
    if ((rc = pt_pass_open(c, v, a.f.r, grid, true, stream))) return rc;
    const uint32_t rounds = (most + PT_FILM_LW - 1u) / PT_FILM_LW;
    for (uint32_t round = 0; round < rounds; round++) {
        PT_HIP(c, pt_film_plan_launch(a.f.r, d_budget, p->max_samples, round, (uint32_t*)f->plan_work.p, list, n_list, stream));
        if (round) PT_HIP(c, hipMemsetAsync((char*)v.misc.p + 256, 0, PT_PASS_MISC_BYTES - 256, stream));  // the queues again; the overflow flag stays
        a.f.r.n_items = bound(round);
        uint32_t g = 0;
        PT_HIP(c, pt_film_map_dispatch(a, k.tex, k.park, c->n_cu, stream, &g, true));  // (g <= grid: no more items than the launch the buffers were sized for)
        PT_HIP(c, pt_film_fold_map_launch(a.f, d_budget, p->max_samples, round, (double*)f->total.p, (double*)f->partial.p, (uint32_t*)f->count.p, f->moments ? (double*)f->q.p : nullptr, stream));
    }
    return pt_pass_seal(c, v);
}

extern "C" int pt_film_add_map(pt_context* c, pt_film* f, const pt_camera* cam, const double* background, const pt_film_map_params* p, const uint32_t* budget, double* kernel_ms) {
    uint32_t most = 0;
    int rc = pt_film_add_map_check(c, f, cam, background, p, budget, budget, &most);
    if (rc) return rc;
    if (kernel_ms) *kernel_ms = 0.0;
    if (most == 0) return PT_OK;  // an inverted slice, or a map of zeros over it: nothing queued, nothing changed
    PT_HIP(c, hipSetDevice(c->device));
    const size_t bg_bytes = (p->background_rows ? (size_t)f->height : (size_t)f->height * f->width) * 24;
    if ((rc = pt_reserve(c, f->bg, bg_bytes)) || (rc = pt_reserve(c, f->budget, f->counts.size() * 4))) return rc;
    PT_HIP(c, hipMemcpy(f->bg.p, background, bg_bytes, hipMemcpyHostToDevice));
    PT_HIP(c, hipMemcpy(f->budget.p, budget, f->counts.size() * 4, hipMemcpyHostToDevice));
    if ((rc = pt_pass_settle(c, c->radiance.pass, pt_film_add_map_common(c, f, cam, (const double*)f->bg.p, p, (const uint32_t*)f->budget.p, most, nullptr)))) return rc;
    for (uint32_t y = p->slice.y0; y <= p->slice.y1; y++) {  // the host's copy of the counts, exactly
        uint32_t* row = f->counts.data() + (size_t)y * f->width;
        const uint32_t* brow = budget + (size_t)y * f->width;
        for (uint32_t x = p->slice.x0; x <= p->slice.x1; x++) row[x] += std::min(brow[x], p->max_samples);
    }
    return pt_pass_result(c, c->radiance.pass, kernel_ms);
}

extern "C" int pt_film_add_map_device(pt_context* c, pt_film* f, const pt_camera* cam, const double* d_background, const pt_film_map_params* p, const uint32_t* d_budget, void* hip_stream) {
    uint32_t most = 0;
    int rc = pt_film_add_map_check(c, f, cam, d_background, p, d_budget, nullptr, &most);
    if (rc) return rc;
    if (most == 0) return PT_OK;  // an inverted slice: nothing queued, nothing to finish
    PT_HIP(c, hipSetDevice(c->device));
    if ((rc = pt_pass_device_tail(c, c->radiance.pass, pt_film_add_map_common(c, f, cam, d_background, p, d_budget, most, (hipStream_t)hip_stream)))) return rc;
    for (uint32_t y = p->slice.y0; y <= p->slice.y1; y++) {  // the host's copy of the counts: an upper bound, until pt_film_counts
        uint32_t* row = f->counts.data() + (size_t)y * f->width;
        for (uint32_t x = p->slice.x0; x <= p->slice.x1; x++) row[x] += p->max_samples;
    }
    c->film_open = f;
    return PT_OK;
}

extern "C" int pt_film_error_device(pt_context* c, pt_film* f, double* d_err, void* hip_stream) {
    if (!c || !f || !d_err) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_error_device: NULL context, film or err");
    int rc = pt_film_handle(c, f, false, "pt_film_error_device");
    if (rc) return rc;
    if (!f->moments) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_error: the film keeps no second moment (pt_film_create_moments)");
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, pt_film_error_launch(f->width, f->height, (const double*)f->total.p, (const double*)f->partial.p, (const uint32_t*)f->count.p, (const double*)f->q.p, d_err, (hipStream_t)hip_stream));
    return PT_OK;
}

extern "C" int pt_film_error(pt_context* c, pt_film* f, double* err) {
    if (!c || !f || !err) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_error: NULL context, film or err");
    int rc = pt_film_handle(c, f, true, "pt_film_error");
    if (rc) return rc;
    if (!f->moments) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_error: the film keeps no second moment (pt_film_create_moments)");
    PT_HIP(c, hipSetDevice(c->device));
    const size_t n = f->counts.size();
    if ((rc = pt_reserve(c, f->out_err, n * 8))) return rc;
    PT_HIP(c, pt_film_error_launch(f->width, f->height, (const double*)f->total.p, (const double*)f->partial.p, (const uint32_t*)f->count.p, (const double*)f->q.p, (double*)f->out_err.p, nullptr));
    PT_HIP(c, hipMemcpy(err, f->out_err.p, n * 8, hipMemcpyDeviceToHost));
    return PT_OK;
}

extern "C" int pt_film_budget_device(pt_context* c, pt_film* f, const pt_film_refine_params* p, uint32_t* d_budget, uint64_t* d_summary, void* hip_stream) {
    if (!c || !f || !p || !d_budget || !d_summary) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_budget_device: NULL context, film, params, budget or summary");
    int rc = pt_film_handle(c, f, true, "pt_film_budget_device");
    if (rc) return rc;
    if (!f->moments) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_budget_device: the film keeps no second moment (pt_film_create_moments)");
    if (p->step == 0 || p->step > PT_FILM_MAP_MAX) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_budget_device: step is 1 .. PT_FILM_MAP_MAX");
    if (p->min_count > p->max_count || p->max_count > PT_FILM_COUNT_MAX) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_budget_device: min_count <= max_count <= 2^31");
    if (p->threshold != p->threshold) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_budget_device: the threshold is not a number");
    if (p->slice.x0 >= f->width || p->slice.x1 >= f->width || p->slice.y0 >= f->height || p->slice.y1 >= f->height)
        return pt_fail(c, PT_ERR_SLICE, "slice corner outside the image (render.rs:79-90)");
    PT_HIP(c, hipSetDevice(c->device));
    PtRenderArgs r;
    memset(&r, 0, sizeof r);
    r.width = f->width; r.height = f->height;
    r.x0 = p->slice.x0; r.y0 = p->slice.y0; r.x1 = p->slice.x1; r.y1 = p->slice.y1;  // (an inverted slice holds no pixel: zeros everywhere)
    PT_HIP(c, hipMemsetAsync(d_summary, 0, 16, (hipStream_t)hip_stream));
    PT_HIP(c, pt_film_budget_launch(r, p->threshold, p->min_count, p->max_count, p->step, (const double*)f->total.p, (const double*)f->partial.p, (const uint32_t*)f->count.p, (const double*)f->q.p,
                                    d_budget, (unsigned long long*)d_summary, (hipStream_t)hip_stream));
    return PT_OK;
}

// ------------------------------------------------------------------------------------------------
// Film, denoised: the a-trous filter over the resolved mean (pt_denoise.h, pt_denoise.hip)
// ------------------------------------------------------------------------------------------------
// Everything that can be refused without a HIP call, in the order the header gives. Bookkeeping is pt_film_resolve_device's, and the call is refused while a
// pass of the film is open.
static int pt_film_denoise_check(pt_context* c, pt_film* f, const pt_denoise_params* p, const pt_denoise_guides* g, const void* rgb, const void* linear, const void* variance, const char* who) {
    if (!c || !f || !p || !g) return pt_fail(c, PT_ERR_ARGUMENT, std::string(who) + ": NULL context, film, params or guides");
    int rc = pt_film_handle(c, f, true, who);
    if (rc) return rc;
    if (const char* why = pt_denoise_check(p, g)) return pt_fail(c, PT_ERR_ARGUMENT, std::string(who) + ": " + why);
    if (!rgb && !linear && !variance) return pt_fail(c, PT_ERR_ARGUMENT, std::string(who) + ": none of rgb, linear and variance");
    if (!f->moments && p->sigma_color > 0.0) return pt_fail(c, PT_ERR_ARGUMENT, std::string(who) + ": the film keeps no second moment (pt_film_create_moments): sigma_color must be 0");
    return PT_OK;
}

// The kernels of one denoise, queued on `stream`: seed, a level kernel per iteration between the film's two work buffers, finish. The context's device is current.
// With an albedo (pt_film_denoise_albedo*) the seed and the finish are pt_denoise_albedo.hip's, the levels the same.
static int pt_film_denoise_queue(pt_context* c, pt_film* f, const pt_denoise_params* p, const pt_denoise_guides& g, const double* d_albedo, uint8_t* d_rgb, double* d_linear, double* d_variance,
                                 hipStream_t stream) {
    const size_t n = f->counts.size();
    int rc;
    if ((rc = pt_reserve(c, f->dn_work[0], n * 32)) || (rc = pt_reserve(c, f->dn_work[1], n * 32))) return rc;
    const bool tiled = pt_env_on("PORTRAYER_DENOISE_TILE", true);  // the LDS-tiled form, the faster one at 5 levels by more than three spreads (profiles/denoise/notes.md), unless the switch says otherwise
    const uint32_t* count = (const uint32_t*)f->count.p;
    const double* q = f->moments ? (const double*)f->q.p : nullptr;
    if (d_albedo) PT_HIP(c, pt_denoise_albedo_seed_launch(f->width, f->height, (const double*)f->total.p, (const double*)f->partial.p, count, q, g.node, d_albedo, (double*)f->dn_work[0].p, stream));
    else PT_HIP(c, pt_denoise_seed_launch(f->width, f->height, (const double*)f->total.p, (const double*)f->partial.p, count, q, (double*)f->dn_work[0].p, stream));
    PtDenoiseLevelArgs a;
    a.k = pt_denoise_const(*p);
    a.width = f->width; a.height = f->height;
    a.count = count;
    a.position = g.position; a.normal = g.normal; a.node = g.node;
    int cur = 0;
    for (int l = 0; l < p->iterations; l++, cur ^= 1) {
        a.step = 1u << l;
        a.in = (const double*)f->dn_work[cur].p;
        a.out = (double*)f->dn_work[cur ^ 1].p;
        PT_HIP(c, pt_denoise_level_launch(a, tiled, stream));
    }
    if (d_albedo) PT_HIP(c, pt_denoise_albedo_finish_launch(f->width, f->height, (const double*)f->dn_work[cur].p, count, g.node, d_albedo, d_rgb, d_linear, d_variance, stream));
    else PT_HIP(c, pt_denoise_finish_launch(f->width, f->height, (const double*)f->dn_work[cur].p, count, d_rgb, d_linear, d_variance, stream));
    return PT_OK;
}

// The device form of both denoises: `who` names the entry point, `albedo` says whether it is the demodulated one (d_albedo is then required).
static int pt_film_denoise_device_any(pt_context* c, pt_film* f, const pt_denoise_params* p, const pt_denoise_guides* d_guides, bool albedo, const double* d_albedo, void* d_rgb, double* d_linear,
                                      double* d_variance, void* hip_stream, const std::string& who) {
    int rc = pt_film_denoise_check(c, f, p, d_guides, d_rgb, d_linear, d_variance, who.c_str());
    if (rc) return rc;
    if (albedo && !d_albedo) return pt_fail(c, PT_ERR_ARGUMENT, who + ": NULL albedo");
    PT_HIP(c, hipSetDevice(c->device));
    const uint64_t n = f->counts.size();
    const bool want_n = p->normal_power_log2 >= 0 || p->sigma_plane > 0.0, want_pos = p->sigma_plane > 0.0;
    pt_denoise_guides g = {want_pos ? d_guides->position : nullptr, want_n ? d_guides->normal : nullptr, d_guides->node};  // (a guide no weight reads is not looked at)
    if ((rc = pt_check_device_pointer(c, g.node, n * 4, who + ": the node guide"))) return rc;
    if (g.normal && (rc = pt_check_device_pointer(c, g.normal, n * 24, who + ": the normal guide"))) return rc;
    if (g.position && (rc = pt_check_device_pointer(c, g.position, n * 24, who + ": the position guide"))) return rc;
    if (d_rgb && (rc = pt_check_device_pointer(c, d_rgb, n * 3, who + ": rgb"))) return rc;
    if (d_linear && (rc = pt_check_device_pointer(c, d_linear, n * 24, who + ": linear"))) return rc;
    if (d_variance && (rc = pt_check_device_pointer(c, d_variance, n * 8, who + ": variance"))) return rc;
    if (albedo && (rc = pt_check_device_pointer(c, d_albedo, n * 24, who + ": the albedo"))) return rc;
    return pt_film_denoise_queue(c, f, p, g, albedo ? d_albedo : nullptr, (uint8_t*)d_rgb, d_linear, d_variance, (hipStream_t)hip_stream);
}

extern "C" int pt_film_denoise_device(pt_context* c, pt_film* f, const pt_denoise_params* p, const pt_denoise_guides* d_guides, void* d_rgb, double* d_linear, double* d_variance,
                                      void* hip_stream) {
    return pt_film_denoise_device_any(c, f, p, d_guides, false, nullptr, d_rgb, d_linear, d_variance, hip_stream, "pt_film_denoise_device");
}

extern "C" int pt_film_denoise_albedo_device(pt_context* c, pt_film* f, const pt_denoise_params* p, const pt_denoise_guides* d_guides, const double* d_albedo, void* d_rgb, double* d_linear,
                                             double* d_variance, void* hip_stream) {
    return pt_film_denoise_device_any(c, f, p, d_guides, true, d_albedo, d_rgb, d_linear, d_variance, hip_stream, "pt_film_denoise_albedo_device");
}

// The host-buffer form of both denoises, as pt_film_denoise_device_any is the device form's.
static int pt_film_denoise_host_any(pt_context* c, pt_film* f, const pt_denoise_params* p, const pt_denoise_guides* host_guides, bool albedo, const double* host_albedo, uint8_t* rgb, double* linear,
                                    double* variance, const std::string& who) {
    int rc = pt_film_denoise_check(c, f, p, host_guides, rgb, linear, variance, who.c_str());
    if (rc) return rc;
    if (albedo && !host_albedo) return pt_fail(c, PT_ERR_ARGUMENT, who + ": NULL albedo");
    PT_HIP(c, hipSetDevice(c->device));
    const size_t n = f->counts.size();
    const bool want_n = p->normal_power_log2 >= 0 || p->sigma_plane > 0.0, want_pos = p->sigma_plane > 0.0;
    pt_denoise_guides g = {nullptr, nullptr, nullptr};
    if ((rc = pt_reserve(c, f->dn_node, n * 4))) return rc;
    PT_HIP(c, hipMemcpy(f->dn_node.p, host_guides->node, n * 4, hipMemcpyHostToDevice));
    g.node = (const int32_t*)f->dn_node.p;
    if (want_n) {
        if ((rc = pt_reserve(c, f->dn_normal, n * 24))) return rc;
        PT_HIP(c, hipMemcpy(f->dn_normal.p, host_guides->normal, n * 24, hipMemcpyHostToDevice));
        g.normal = (const double*)f->dn_normal.p;
    }
    if (want_pos) {
        if ((rc = pt_reserve(c, f->dn_position, n * 24))) return rc;
        PT_HIP(c, hipMemcpy(f->dn_position.p, host_guides->position, n * 24, hipMemcpyHostToDevice));
        g.position = (const double*)f->dn_position.p;
    }
    const double* d_albedo = nullptr;
    if (albedo) {
        if ((rc = pt_reserve(c, f->dn_albedo, n * 24))) return rc;
        PT_HIP(c, hipMemcpy(f->dn_albedo.p, host_albedo, n * 24, hipMemcpyHostToDevice));
        d_albedo = (const double*)f->dn_albedo.p;
    }
    // pixels without samples keep the caller's bytes: where there are any, the caller's buffers go to the device first (pt_film_resolve)
    PT_HIP(c, hipMemcpy(f->counts.data(), f->count.p, n * 4, hipMemcpyDeviceToHost));  // (behind a device map the host's copy is an upper bound)
    const bool holes = std::find(f->counts.begin(), f->counts.end(), 0u) != f->counts.end();
    if (rgb) {
        if ((rc = pt_reserve(c, f->out_rgb, n * 3))) return rc;
        if (holes) PT_HIP(c, hipMemcpy(f->out_rgb.p, rgb, n * 3, hipMemcpyHostToDevice));
    }
    if (linear) {
        if ((rc = pt_reserve(c, f->out_linear, n * 24))) return rc;
        if (holes) PT_HIP(c, hipMemcpy(f->out_linear.p, linear, n * 24, hipMemcpyHostToDevice));
    }
    if (variance) {
        if ((rc = pt_reserve(c, f->out_var, n * 8))) return rc;
        if (holes) PT_HIP(c, hipMemcpy(f->out_var.p, variance, n * 8, hipMemcpyHostToDevice));
    }
    if ((rc = pt_film_denoise_queue(c, f, p, g, d_albedo, rgb ? (uint8_t*)f->out_rgb.p : nullptr, linear ? (double*)f->out_linear.p : nullptr, variance ? (double*)f->out_var.p : nullptr, nullptr))) return rc;
    if (rgb) PT_HIP(c, hipMemcpy(rgb, f->out_rgb.p, n * 3, hipMemcpyDeviceToHost));
    if (linear) PT_HIP(c, hipMemcpy(linear, f->out_linear.p, n * 24, hipMemcpyDeviceToHost));
    if (variance) PT_HIP(c, hipMemcpy(variance, f->out_var.p, n * 8, hipMemcpyDeviceToHost));
    return PT_OK;
}

extern "C" int pt_film_denoise(pt_context* c, pt_film* f, const pt_denoise_params* p, const pt_denoise_guides* host_guides, uint8_t* rgb, double* linear, double* variance) {
    return pt_film_denoise_host_any(c, f, p, host_guides, false, nullptr, rgb, linear, variance, "pt_film_denoise");
}

extern "C" int pt_film_denoise_albedo(pt_context* c, pt_film* f, const pt_denoise_params* p, const pt_denoise_guides* host_guides, const double* albedo, uint8_t* rgb, double* linear,
                                      double* variance) {
    return pt_film_denoise_host_any(c, f, p, host_guides, true, albedo, rgb, linear, variance, "pt_film_denoise_albedo");
}

// The plan kernels alone (tests): the list of one launch round, copied back.
extern "C" int pt_test_film_plan(pt_context* c, uint32_t width, uint32_t height, const pt_rect* slice, const uint32_t* budget, uint32_t max_samples, uint32_t round, uint32_t* list, uint32_t cap,
                                 uint32_t* n_out) {
    if (!c || !slice || !budget || !n_out || (!list && cap) || width == 0 || height == 0 || (uint64_t)width * height >= 0x80000000ull || max_samples == 0 || max_samples > PT_FILM_MAP_MAX ||
        round >= (PT_FILM_MAP_MAX + PT_FILM_LW - 1) / PT_FILM_LW)
        return pt_fail(c, PT_ERR_ARGUMENT, "pt_test_film_plan: bad argument");
    if (slice->x0 > slice->x1 || slice->y0 > slice->y1 || slice->x1 >= width || slice->y1 >= height) return pt_fail(c, PT_ERR_SLICE, "pt_test_film_plan: bad slice");
    if (pt_film_slice_slots(*slice) >= PT_FILM_MAP_SLOTS_MAX) return pt_fail(c, PT_ERR_ARGUMENT, "pt_test_film_plan: a slice of 2^29 pixel slots or more");
    PT_HIP(c, hipSetDevice(c->device));
    PtRenderArgs r;
    memset(&r, 0, sizeof r);
    r.width = width; r.height = height;
    r.x0 = slice->x0; r.y0 = slice->y0; r.x1 = slice->x1; r.y1 = slice->y1;
    r.tile_rank = 0; r.tile_ranks = 1;
    r.n_slots = (uint32_t)pt_film_slice_slots(*slice);
    const size_t n_pixels = (size_t)width * height;
    PtBuf d_budget, d_list, d_work;
    int rc;
    if ((rc = pt_reserve(c, d_budget, n_pixels * 4)) || (rc = pt_reserve(c, d_list, 16 + (size_t)r.n_slots * PT_FILM_LW * 4)) || (rc = pt_reserve(c, d_work, pt_film_plan_words(r.n_slots) * 4))) return rc;
    uint32_t n = 0;
    hipError_t e = hipMemcpy(d_budget.p, budget, n_pixels * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = pt_film_plan_launch(r, (const uint32_t*)d_budget.p, max_samples, round, (uint32_t*)d_work.p, (uint32_t*)((char*)d_list.p + 16), (uint32_t*)d_list.p, nullptr);
    if (e == hipSuccess) e = hipMemcpy(&n, d_list.p, 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && n > r.n_slots * (uint32_t)PT_FILM_LW) n = r.n_slots * (uint32_t)PT_FILM_LW;  // (never: the list's room)
    if (e == hipSuccess && std::min(n, cap)) e = hipMemcpy(list, (char*)d_list.p + 16, (size_t)std::min(n, cap) * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return pt_fail(c, PT_ERR_DEVICE, std::string("pt_test_film_plan: ") + hipGetErrorString(e));
    *n_out = n;
    return PT_OK;
}

// ------------------------------------------------------------------------------------------------
// Harness helpers
// ------------------------------------------------------------------------------------------------
extern "C" int pt_device_alloc(pt_context* c, uint64_t bytes, void** out) {
    if (!c || !out) return PT_ERR_ARGUMENT;
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipMalloc(out, bytes ? bytes : 16));
    return PT_OK;
}
extern "C" int pt_device_free(pt_context* c, void* p) {
    if (!c) return PT_ERR_ARGUMENT;
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipFree(p));
    return PT_OK;
}
extern "C" int pt_copy_to_device(pt_context* c, void* dst, const void* src, uint64_t bytes) {
    if (!c) return PT_ERR_ARGUMENT;
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return PT_OK;
}
extern "C" int pt_copy_from_device(pt_context* c, void* dst, const void* src, uint64_t bytes) {
    if (!c) return PT_ERR_ARGUMENT;
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return PT_OK;
}

extern "C" int pt_synchronize(pt_context* c) {
    if (!c) return PT_ERR_ARGUMENT;
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipDeviceSynchronize());
    return PT_OK;
}

extern "C" int pt_measure_copy_bandwidth(pt_context* c, uint64_t bytes, int iters, double* gbps) {
    if (!c || !gbps || bytes < 16) return PT_ERR_ARGUMENT;
    PT_HIP(c, hipSetDevice(c->device));
    void *src = nullptr, *dst = nullptr;
    PT_HIP(c, hipMalloc(&src, bytes));
    PT_HIP(c, hipMalloc(&dst, bytes));
    PT_HIP(c, hipMemset(src, 1, bytes));
    size_t n = bytes / 16;
    double best = 0.0;
    // The box's copy roofline = the best of a few ways to copy: a grid-stride kernel with four loads in flight at four grid
    // sizes, one element per thread, and the runtime's own device-to-device copy.
    const int per_cu[4] = {8, 16, 32, 64};
    for (int i = 0; i < 6 * iters + 1; i++) {
        const int form = i % 6;
        PT_HIP(c, hipEventRecord(c->slot[0].ev0, nullptr));
        if (form < 4) hipLaunchKernelGGL(pt_copy_kernel, dim3(c->n_cu * per_cu[form]), dim3(256), 0, nullptr, (const double2*)src, (double2*)dst, n);
        else if (form == 4) hipLaunchKernelGGL(pt_copy1_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, (const double2*)src, (double2*)dst, n);
        else PT_HIP(c, hipMemcpyAsync(dst, src, n * 16, hipMemcpyDeviceToDevice, nullptr));
        PT_HIP(c, hipEventRecord(c->slot[0].ev1, nullptr));
        PT_HIP(c, hipEventSynchronize(c->slot[0].ev1));
        float ms = 0.f;
        PT_HIP(c, hipEventElapsedTime(&ms, c->slot[0].ev0, c->slot[0].ev1));
        if (i > 0 && ms > 0.f) {
            const double rate = 2.0 * (double)(n * 16) / (ms * 1e-3) / 1e9;
            if (pt_env_set("PORTRAYER_VERBOSE")) fprintf(stderr, "[pt_measure_copy_bandwidth] form %d: %.0f GB/s\n", form, rate);
            best = std::max(best, rate);
        }
    }
    hipFree(src); hipFree(dst);
    *gbps = best;
    return PT_OK;
}

extern "C" int pt_test_cast_rays(pt_context* c, uint64_t n, const double* origins, const double* directions, int any_hit,
                                 double* out_t, int32_t* out_node, int32_t* out_sub) {
    if (!c || !origins || !directions || !out_t || !out_node || !out_sub) return PT_ERR_ARGUMENT;
    if (!c->have_scene) return pt_fail(c, PT_ERR_NO_SCENE, "no scene uploaded");
    if (n == 0) return PT_OK;
    PT_HIP(c, hipSetDevice(c->device));
    struct Bufs {  // freed on every return path
        void* p[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        ~Bufs() { for (void* q : p) if (q) hipFree(q); }
    } bufs;
    const size_t sizes[5] = {n * 24, n * 24, n * 8, n * 4, n * 4};
    for (int k = 0; k < 5; k++) PT_HIP(c, hipMalloc(&bufs.p[k], sizes[k]));
    double *d_o = (double*)bufs.p[0], *d_d = (double*)bufs.p[1], *d_t = (double*)bufs.p[2];
    int32_t *d_n = (int32_t*)bufs.p[3], *d_s = (int32_t*)bufs.p[4];
    int rc = pt_reserve(c, c->misc, 256 + sizeof(PtCounters));
    if (rc) return rc;
    PT_HIP(c, hipMemset(c->misc.p, 0, 8));
    unsigned int* overflow = (unsigned int*)c->misc.p + 1;
    PT_HIP(c, hipMemcpy(d_o, origins, n * 24, hipMemcpyHostToDevice));
    PT_HIP(c, hipMemcpy(d_d, directions, n * 24, hipMemcpyHostToDevice));
    size_t lds = (size_t)c->view.stack_cap * PT_BLOCK * 4;
    if (lds > 160 * 1024) return pt_fail(c, PT_ERR_SCENE, "pt_test_cast_rays keeps the whole traversal stack in LDS: tree too deep for it");
    dim3 grid((unsigned)((n + PT_BLOCK - 1) / PT_BLOCK));
    auto cast = [&](auto mode) -> hipError_t {
        constexpr int M = decltype(mode)::value;
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&pt_cast_kernel<M>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(pt_cast_kernel<M>, grid, dim3(PT_BLOCK), lds, nullptr, c->view, n, d_o, d_d, any_hit, d_t, d_n, d_s, overflow);
        return hipSuccess;
    };
    switch (c->view.mode) {
    case PT_MODE_FLAT_NOMESH: PT_HIP(c, cast(std::integral_constant<int, PT_MODE_FLAT_NOMESH>())); break;
    case PT_MODE_KD: PT_HIP(c, cast(std::integral_constant<int, PT_MODE_KD>())); break;
    case PT_MODE_FLAT_KDMESH: PT_HIP(c, cast(std::integral_constant<int, PT_MODE_FLAT_KDMESH>())); break;
    case PT_MODE_HIER: PT_HIP(c, cast(std::integral_constant<int, PT_MODE_HIER>())); break;
    case PT_MODE_HIER_NOMESH: PT_HIP(c, cast(std::integral_constant<int, PT_MODE_HIER_NOMESH>())); break;
    case PT_MODE_KD_NOMESH: PT_HIP(c, cast(std::integral_constant<int, PT_MODE_KD_NOMESH>())); break;
    case PT_MODE_HIER_MESH: PT_HIP(c, cast(std::integral_constant<int, PT_MODE_HIER_MESH>())); break;
    case PT_MODE_KD_MESH: PT_HIP(c, cast(std::integral_constant<int, PT_MODE_KD_MESH>())); break;
    default: PT_HIP(c, cast(std::integral_constant<int, PT_MODE_FLAT>())); break;
    }
    PT_HIP(c, hipGetLastError());
    PT_HIP(c, hipDeviceSynchronize());
    PT_HIP(c, hipMemcpy(out_t, d_t, n * 8, hipMemcpyDeviceToHost));
    PT_HIP(c, hipMemcpy(out_node, d_n, n * 4, hipMemcpyDeviceToHost));
    PT_HIP(c, hipMemcpy(out_sub, d_s, n * 4, hipMemcpyDeviceToHost));
    unsigned int head[2] = {0, 0};
    PT_HIP(c, hipMemcpy(head, c->misc.p, sizeof head, hipMemcpyDeviceToHost));
    if (head[1] & 4u) return pt_fail(c, PT_ERR_TRAVERSAL, "a tree walk did not end (watchdog): results invalid");
    if (head[1]) return pt_fail(c, PT_ERR_TRAVERSAL, "traversal stack overflow");
    return PT_OK;
}

extern "C" int pt_test_pow_host(uint64_t n, const double* x, const double* y, double* port, double* libm) {
    if (!x || !y || !port || !libm) return PT_ERR_ARGUMENT;
    for (uint64_t i = 0; i < n; i++) { port[i] = pt_pow_glibc(x[i], y[i]); libm[i] = pow(x[i], y[i]); }
    return PT_OK;
}

// The HOST's libm (glibc: what the reference and the oracle call) on explicit inputs, op numbered like pt_test_math: 2 pow, 4 atan2, 5 acos.
// (numpy's vectorised routines are not libm's on every machine: tests compare the device with this.)
extern "C" int pt_test_libm_host(int op, uint64_t n, const double* a, const double* b, double* out) {
    if (!a || !b || !out) return PT_ERR_ARGUMENT;
    for (uint64_t i = 0; i < n; i++) {
        switch (op) {
        case 2: out[i] = pow(a[i], b[i]); break;
        case 4: out[i] = atan2(a[i], b[i]); break;
        case 5: out[i] = acos(a[i]); break;
        default: return PT_ERR_ARGUMENT;
        }
    }
    return PT_OK;
}

extern "C" int pt_test_math(pt_context* c, int op, uint64_t n, const double* a, const double* b, double* out) {
    if (!c || !a || !b || !out) return PT_ERR_ARGUMENT;
    if (n == 0) return PT_OK;
    PT_HIP(c, hipSetDevice(c->device));
    struct Bufs {
        void* p[3] = {nullptr, nullptr, nullptr};
        ~Bufs() { for (void* q : p) if (q) hipFree(q); }
    } bufs;
    for (int k = 0; k < 3; k++) PT_HIP(c, hipMalloc(&bufs.p[k], n * 8));
    double *d_a = (double*)bufs.p[0], *d_b = (double*)bufs.p[1], *d_o = (double*)bufs.p[2];
    PT_HIP(c, hipMemcpy(d_a, a, n * 8, hipMemcpyHostToDevice));
    PT_HIP(c, hipMemcpy(d_b, b, n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(pt_math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, op, n, d_a, d_b, d_o);
    PT_HIP(c, hipGetLastError());
    PT_HIP(c, hipDeviceSynchronize());
    PT_HIP(c, hipMemcpy(out, d_o, n * 8, hipMemcpyDeviceToHost));
    return PT_OK;
}
