// The C ABI declared in include/portrayer_hip.h: context, scene upload (tree builds), render calls, and the
// small kernels around the render kernel (finishing pass, untile, explicit-ray casts for the parity tests).
// The render kernel itself is in pt_render_kernel.h, instantiated per traversal mode by pt_render_inst.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/portrayer_hip.h"
#include "pt_build.h"
#include "pt_bvh.h"
#include "pt_aov_inst.h"
#include "pt_guides_inst.h"
#include "pt_rays_inst.h"
#include "pt_segments_inst.h"
#include "pt_ao_inst.h"
#include "pt_radiance_inst.h"
#include "pt_gather_inst.h"
#include "pt_film_inst.h"
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

// Two-child tree -> four-child tree (PtBvh4Node, pt_scene_view.h). Node i starts with its two children and, while it has
// fewer than four, replaces the inner child with the largest surface area by that child's two children (the child a ray is
// most likely to enter is the one worth opening; taking over both children's children regardless leaves a node with a leaf
// child at three entries). Mesh trees only: on scene-level trees the grandchildren form measured better (transmission-refraction
// 3.32 against 3.72 node visits per ray). PORTRAYER_COLLAPSE=plain | mesh | area.
// One thread per two-child node; entries of the array that no tree uses (the device build reserves n - 1 nodes per mesh
// and may need fewer) are never referenced and are only kept from reading out of bounds. In a device-built tree's place they
// hold 0xFF bytes, i.e. PT_REF_EMPTY children: pt_scene_upload and a rebuild by pt_scene_deform fill the place before the
// builder runs, and pt_parent_kernel / pt_refit_kernel (pt_build.hip), which scan the whole place, rely on that - the memset is not redundant.
// tri_leaf: the edge record of every triangle named by a slot of the items array, in slot order (80 bytes a slot: 9 f64 + the triangle's index), so
// that a mesh leaf's triangles lie side by side and the wave-uniform walks fetch them without going through bvh_items first.
__global__ void __launch_bounds__(256) pt_tri_leaf_kernel(const uint32_t* __restrict__ items, uint32_t n_items, const double* __restrict__ tri_e, uint32_t n_tris,
                                                         double* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_items) return;
    const uint32_t t = items[i];
    double* o = out + 10 * (size_t)i;
    if (t < n_tris) {
        const double* e = tri_e + 9 * (size_t)t;
        for (int k = 0; k < 9; k++) o[k] = e[k];
    } else {
        for (int k = 0; k < 9; k++) o[k] = 0.0;
    }
    union { double d; uint32_t u[2]; } c; c.u[0] = t; c.u[1] = 0u;
    o[9] = c.d;
}

// [first, end): the nodes this launch converts (pt_scene_upload: all n of them; pt_scene_update: the scene-level tree's alone).
__global__ void __launch_bounds__(256) pt_collapse4_kernel(const PtBvhNode* __restrict__ bvh2, PtBvh4Node* __restrict__ bvh4, uint32_t n, int by_area_mode,
                                                            uint32_t scene_first, uint32_t scene_end, uint32_t first, uint32_t end) {
    const uint32_t i = first + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= end || i >= n) return;
    // by_area_mode 0: never, 1: mesh trees only (nodes outside [scene_first, scene_end)), 2: every tree
    const bool by_area = by_area_mode == 2 || (by_area_mode == 1 && (i < scene_first || i >= scene_end));
    const PtBvhNode a = bvh2[i];
    float lo[4][3], hi[4][3];
    uint32_t child[4];
    int k = 0;
    auto put = [&](const PtBvhNode& nd, int which) {
        pt_node_get_box(nd, which, lo[k], hi[k]);
        child[k] = which ? nd.child1 : nd.child0;
        k++;
    };
    auto inner = [&](uint32_t c) { return c != PT_REF_EMPTY && !(c & PT_REF_LEAF) && c < n; };
    if (by_area) {
        if (a.child0 != PT_REF_EMPTY) put(a, 0);
        if (a.child1 != PT_REF_EMPTY) put(a, 1);
        while (k < 4) {
            int best = -1;
            float best_area = -1.0f;
            for (int j = 0; j < k; j++) {
                if (!inner(child[j])) continue;
                const float dx = hi[j][0] - lo[j][0], dy = hi[j][1] - lo[j][1], dz = hi[j][2] - lo[j][2];
                const float area = dx * dy + dy * dz + dz * dx;
                if (!(area <= best_area)) { best = j; best_area = area; }  // also takes a NaN / infinite area rather than nothing
            }
            if (best < 0) break;
            const PtBvhNode c = bvh2[child[best]];
            const int n_kids = (c.child0 != PT_REF_EMPTY) + (c.child1 != PT_REF_EMPTY);
            if (n_kids == 0) { child[best] = child[k - 1]; for (int ax = 0; ax < 3; ax++) { lo[best][ax] = lo[k - 1][ax]; hi[best][ax] = hi[k - 1][ax]; } k--; continue; }
            // the first child takes the opened entry's place, the second goes to the end
            const int first = c.child0 != PT_REF_EMPTY ? 0 : 1;
            pt_node_get_box(c, first, lo[best], hi[best]);
            child[best] = first ? c.child1 : c.child0;
            if (n_kids == 2) put(c, 1);
        }
    } else {
        auto expand = [&](const PtBvhNode& nd, int which) {
            const uint32_t c0 = which ? nd.child1 : nd.child0;
            if (c0 == PT_REF_EMPTY) return;
            if (!inner(c0)) { put(nd, which); return; }
            const PtBvhNode c = bvh2[c0];
            if (c.child0 != PT_REF_EMPTY) put(c, 0);
            if (c.child1 != PT_REF_EMPTY) put(c, 1);
        };
        expand(a, 0);
        expand(a, 1);
    }
    PtBvh4Node o;
    for (int j = 0; j < 4; j++) {
        const bool used = j < k;
        for (int ax = 0; ax < 3; ax++) { o.lo[ax][j] = used ? lo[j][ax] : (float)PT_BOX_LIMIT; o.hi[ax][j] = used ? hi[j][ax] : -(float)PT_BOX_LIMIT; }
        o.child[j] = used ? child[j] : PT_REF_EMPTY;
    }
    o.pad[0] = o.pad[1] = o.pad[2] = o.pad[3] = 0u;
    bvh4[i] = o;
}

// Second pass of a render: chunk sums -> pixels, a block of PT_BLOCK threads per PT_BLOCK pixel slots. The chunk sums are pixel-major (the
// render kernel's chunk-first lanes write one pixel's sums side by side), so a thread per pixel would read 24 bytes every 24 x n_chunks
// bytes; instead the block first adds them up EIGHT THREADS PER PIXEL - thread j of a pixel holds chunk 8 b + j of the b-th block of eight,
// its seven neighbours' loads next to it, and the pixel's first thread adds the eight values in ascending order (the summation contract: a
// fixed left-to-right association) - leaves the sums in LDS, and then finishes ONE pixel per thread (the three pows with every lane busy).
__global__ void __launch_bounds__(PT_BLOCK) pt_finish_kernel(PtRenderArgs a) {
    __shared__ double sums[3 * PT_BLOCK];
    const uint32_t base = blockIdx.x * PT_BLOCK, j = threadIdx.x & 7u;
    for (uint32_t pass = 0; pass < 8u; pass++) {
        const uint32_t local = pass * (PT_BLOCK / 8u) + (threadIdx.x >> 3), p = base + local;
        PtVec3 sum = pt_v3(0.0, 0.0, 0.0);
        for (uint32_t b = 0; b < a.n_chunks; b += 8u) {  // (wave-uniform trip count)
            const uint32_t k = b + j;
            PtVec3 v = pt_v3(0.0, 0.0, 0.0);
            if (p < a.n_slots && k < a.n_chunks) { const double* c = a.accum + 3 * ((size_t)p * a.n_chunks + k); v = pt_v3(c[0], c[1], c[2]); }
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
    if (p < a.n_slots) pt_finish_pixel(a, p, pt_v3(sums[3 * threadIdx.x], sums[3 * threadIdx.x + 1], sums[3 * threadIdx.x + 2]));
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

// PORTRAYER_OCC_SEED (tests only, pt_render_common): the occluder table filled with hints the test chooses instead of zeros - every entry
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

// The launch's per-pixel candidate lists (pt_pixel_list.h), behind the eye table and the certain-shadow table: a wavefront per 8x8 tile of the launch's own tiles, a lane
// per pixel slot - pixels of partial tiles outside the slice get a record like any other. The 64 beams of a tile reach nearly the same nodes, so ONE walk of sc.bvh
// serves them: a node is entered when any lane's beam reaches its box (a lane whose beam missed the box above tests the children all the same: a leaf too many in a list
// changes nothing), the pending nodes are one list per wavefront in LDS, and a child that is a leaf goes straight into the lists of the lanes that reach it - every item of
// it with the leaf box's bound. A lane's list is its LDS column, kept sorted (pt_pl_insert). A stack that runs full marks the tile's 64 records "take the walk".
// cap (PORTRAYER_PIXEL_LIST_CAP, tests only): entries a list may hold, <= PT_PL_K.
#define PT_PL_BLOCK 256
#define PT_PL_STACK 64
__global__ void __launch_bounds__(PT_PL_BLOCK) pt_pixel_list_kernel(PtRenderArgs a, uint32_t* __restrict__ table, uint32_t cap) {
    __shared__ uint32_t s_list[PT_PL_BLOCK / 64][PT_PL_K][64];
    __shared__ uint32_t s_stack[PT_PL_BLOCK / 64][PT_PL_STACK];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t tile_local = blockIdx.x * (PT_PL_BLOCK / 64) + wave;
    if (tile_local >= a.n_slots / 64u) return;  // (wave-uniform)
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

// ------------------------------------------------------------------------------------------------
// Context
// ------------------------------------------------------------------------------------------------
// A device buffer (pt_reserve). It dies with its owner - the context, a film, a function's scope - whose device is current wherever one is destroyed.
struct PtBuf {
    void* p = nullptr;
    size_t bytes = 0;
    PtBuf() = default;
    PtBuf(const PtBuf&) = delete;
    PtBuf& operator=(const PtBuf&) = delete;
    ~PtBuf() { if (p) hipFree(p); }
};

// What a device pass beside the render owns whatever its kind (primary visibility, ray queries, radiance and the film's passes; the pt_pass_* functions below),
// so that the two render slots stay as they are whatever is in flight on them, and every pass whatever is in flight on another.
struct PtPass {
    PtBuf stack_spill;                         // the lanes' HBM stack columns
    PtBuf spill;                               // the lanes' recursion-frame lines (the radiance pass and the film's only)
    PtBuf misc;                                // the overflow flag (word 1, where a render has it) and, from +256 on, the work queues
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // around the kernels (kernel_ms)
    hipEvent_t copy_done = nullptr;            // behind the copy into `host`
    unsigned char* host = nullptr;             // pinned: the first two words of misc (the second is the overflow flag)
    hipStream_t stream = nullptr;              // of the last pass queued
    bool pending = false;                      // a _device call not yet closed by its _finish
    bool queued = false;                       // something of the last pass queued may still be in flight (pt_pass_wait)
    bool closed = false;                       // ... and all of it was queued: copy_done is recorded behind it
};
// What reorder = 1 of the ray passes sorts with: keys and ray indices before and after, the sort's scratch (pt_ray_sort_reserve, pt_ray_sort_queue).
struct PtRaySort {
    PtBuf keys[2], vals[2], tmp;
    size_t tmp_bytes = 0;
};

struct pt_film;
struct pt_context {
    int device = 0;
    int n_cu = 0;
    std::string err;
    PtBuf inv, fwd, nrm, info, tri_v, tri_e, tri_leaf, tri_n, meshes, materials, lights, bvh, bvh4, bvh_items, kd, kd_items;
    PtBuf mat_maps, uv_trans, tex, tex_rgb, srgb_lut, tri_uv, texview, mkd, mkd_items;
    PtBuf node_box, kd_box, mkd_box, mkd_item_box, kd_ref;
    PtBuf g_inv, g_fwd, g_nrm, chain_off, chain, dfs_rank, hier_rec, own_inv;  // PT_TRAVERSE_HIER: the scene graph
    PtBuf bg, rgb, linear, misc;  // (pt_render's host-buffer path; misc: pt_test_cast_rays' overflow flag)
    bool needs_spill = false;  // some material is reflective (recursion frames) or the scene has more than 32 lights
    bool spawns = false;       // some material is reflective: hits spawn rays, so the cost of a pixel varies by orders of magnitude
    bool one_ray = false;      // ... and every reflective material is opaque (no index of refraction): a hit spawns at most one ray, the recursion is a chain
    bool forkable = false;     // ... and no hit draws random numbers after the jitter (no area light, no glossy material): refracted subtrees may be walked by other lanes
    uint32_t launch_seq = 0;   // PtRenderArgs::launch_nonce
    bool four_waves_untextured = false;  // ... or, while the scene has no texture maps: any scene with plain Mesh instances
    bool four_waves_hier = false;        // ... or any scene without KDMesh trees in the hierarchical semantics
    bool four_waves = false;   // traversal-heavy scene without reflective materials, flat_scene / hierarchical semantics: a kernel compiled for more than 3 waves per SIMD
    bool five_waves = false;   // ... mesh-free: 5 waves per SIMD (96 registers)
    bool five_waves_mesh = false;  // ... very many triangles in plain Mesh instances, untextured: 5 waves too
    PtSceneView view;
    bool have_scene = false;
    // Up to PT_SLOTS renders of one context may be in flight on a stream (pt_render_device ... pt_render_finish, oldest first): a frame's
    // events and the page of pinned host memory its overflow flag and counters are copied to - asynchronously, right behind its kernels -
    // belong to its slot, so closing a frame is an event wait and a read of host memory: no blocking copy, and the next frame may already
    // be queued behind it (pt_node: frame k + 1 renders while frame k is gathered).
    // Round 5: a slot also owns the launch's WORK buffers (chunk sums, recursion frames, stack overflow columns, work counters / queues / statistics) and a
    // stream of its own (pt_context_stream), so that two frames may be in flight on two queues at once: the render kernels are persistent - a launch's
    // wavefronts retire one by one over the duration of its longest work items (the TAIL: 0.13 ms of a 1.3 ms share of the headline frame, 11 %;
    // profiles/r05/notes.md section 2) - and the next frame's wavefronts take the places they free instead of waiting for the last one.
    struct Slot {
        PtBuf spill, stack_spill, accum, misc;     // misc: work counter + overflow flag (8 B), PtCounters at +256, the work queues behind them
        PtBuf eye_tab;                             // the launch's eye table (pt_eye_table_kernel): n_nodes x 96 bytes, the slot's own - the other slot's frame has another camera;
                                                   // behind it the launch's certain-shadow table (pt_certain_table_kernel): n_nodes x 16 bytes
        hipStream_t stream = nullptr;              // pt_context_stream(ctx, slot): non-blocking, created with the context
        hipEvent_t ev0 = nullptr, ev1 = nullptr;   // around the kernels (pt_stats.kernel_ms)
        hipEvent_t copy_done = nullptr;            // behind the copy into `host`
        unsigned char* host = nullptr;   // pinned: [0, 8) work counter + overflow flag, [256, 256 + sizeof(PtCounters)) the counters
        bool pending = false, counted = false;
        uint32_t mode = 0, variant = 0;  // pt_stats.kernel_mode / kernel_variant of the launch
        std::chrono::steady_clock::time_point t_start;
    };
    static constexpr int PT_SLOTS = 2;
    Slot slot[PT_SLOTS];
    int slot_next = 0;     // the slot the next launch takes
    int slot_oldest = 0;   // the oldest launch not yet closed (== slot_next: none, unless every slot is pending)
    uint32_t last_mode = 0, last_variant = 0;
    int pl_slot = -1;          // pt_test_pixel_list_summary: the slot whose eye_tab buffer holds the last launch's pixel lists (-1: that launch had none) ...
    uint32_t pl_slots = 0;     // ... its pixel slots ...
    size_t pl_off = 0;         // ... and where its records start in the buffer
    // The three passes beside the render, each with a PtPass of its own: all three may be in flight at once, with two renders. Beside it, what is the kind's.
    // The primary-visibility pass (pt_aov / pt_aov_device ... pt_aov_finish): the device copies of the host-buffer path's six outputs.
    // The guides pass (pt_guides ...) runs on the SAME pass - one of the two in flight, one set of stack columns - and its host-buffer path takes position, normal and
    // node from out[1 .. 3] and the albedo from a buffer of its own.
    struct Aov {
        PtPass pass;
        PtBuf out[6];
        PtBuf albedo;
        bool guides = false;  // the pass in flight (pass.pending) is a pt_guides_device one: which words a refusal uses
    } aov;
    // The ray-query pass (pt_rays / pt_segments, their _device forms ... pt_rays_finish): the device copies of the host-buffer path's inputs (in_t_max: pt_segments'
    // third) and seven outputs.
    struct Rays {
        PtPass pass;
        PtBuf in[2], in_t_max, out[7];
        PtRaySort sort;
    } rays;
    // The radiance pass (pt_radiance / pt_radiance_device ... pt_radiance_finish), which a film's passes share: the device copies of the host-buffer path's three
    // inputs and its output.
    struct Radiance {
        PtPass pass;
        PtBuf in[3], out;
        PtRaySort sort;
    } radiance;
    PtPass* const passes[3] = {&aov.pass, &rays.pass, &radiance.pass};
    // Films (pt_film_create): each owns its device state; a film pass is a radiance pass for bookkeeping (pt_film_add_device), film_open names the film of the
    // one in flight. Films still alive die with the context.
    std::vector<pt_film*> films;
    pt_film* film_open = nullptr;
    // What pt_scene_update needs of the uploaded scene besides the device buffers: everything a flattened node's world box is made of apart from its
    // matrix, the node paths (identity bits of hier_rec, own_inv), where the scene-level tree sits in bvh / bvh4 (bvh_items with PORTRAYER_TLAS_LEAF != 1),
    // and the figures stack_cap and forkable are derived from.
    struct Resident {
        int traverse = 0;
        uint32_t n_nodes = 0, n_graph = 0, n_lights = 0;
        std::vector<uint32_t> info;            // 4 words per flattened node, as uploaded
        std::vector<PtBuildBox> mesh_box;      // per mesh: the padded model box
        std::vector<PtBuildBox> tri_box;       // per stand-alone triangle: the padded model box
        size_t mesh_tris = 0;                  // stand-alone triangle t is triangle mesh_tris + t
        std::vector<uint32_t> chain_off, chain;
        size_t tlas_first = 0, tlas_cap = 0;   // the scene-level tree's nodes: bvh[tlas_first, tlas_first + tlas_cap), tlas_cap = n_nodes - 1
        size_t tlas_items = 0;                 // ... and its n_nodes leaf items in bvh_items (none when the leaves are direct)
        size_t tree_nodes = 0;                 // nodes in bvh / bvh4 altogether
        int tlas_leaf = 1, collapse_mode = 1;
        int below = 0;                         // stack_cap: the deepest walk under a scene leaf
        int last_builder = 0, last_rounds = 0; // tests: who built the scene-level tree last (0 the upload, 1 an update on the host, 2 on the device) and in how many clustering rounds
        bool mat_draws = false, dielectric = false;  // forkable: what the materials say
        // pt_scene_deform: where every mesh's tree sits in bvh / bvh4 (nodes) and bvh_items / tri_leaf (items), who built it and how deep it is; the
        // meshes' indices as uploaded (they go to the device with the first deform) and the PtMeshInfo records (bbox_inv and blas_root change)
        struct MeshPlace {
            uint32_t node_first = 0, node_count = 0, item_first = 0, item_count = 0, n_verts = 0;
            int depth = 0;                 // of the two-child tree
            bool device_built = false;     // its place has the device builder's worst-case size: it can be rebuilt there
            bool has_normals = false;
            bool parents_valid = false;    // tree_parent holds this tree's parents (set by the first refit, cleared by a rebuild)
        };
        std::vector<MeshPlace> place;
        std::vector<uint32_t> indices;
        std::vector<PtMeshInfo> meshes;
        bool indices_resident = false;     // mesh_idx holds `indices`
        int blas_leaf = 2, max_kdm_depth = 0;
        bool any_normals = false;          // tri_n holds a record per triangle (some node shades smoothly)
    } res;
    PtBuf mesh_box_dev;  // the per-mesh boxes again, 6 f64 each, for the device build of the scene-level tree
    // pt_scene_deform, allocated by the first deform of the context: the meshes' indices, a parent index and an arrival counter per tree node (the refit),
    // and the staging buffer the new vertices are copied to
    PtBuf mesh_idx, tree_parent, tree_arrive, deform_stage;
    PtBuf vbox;  // pt_vertex_bounds_device / pt_scene_deform_device: the reduction's per-block partials (PtVboxPartial); a work buffer, not part of the scene
    double root_lo[3] = {0.0, 0.0, 0.0}, root_hi[3] = {0.0, 0.0, 0.0};  // the scene tree's root box: union of the flattened nodes' world boxes (reorder = 1 quantises origins inside it)
};
#define PT_SLOT_BYTES (256 + sizeof(PtCounters))

// A film (include/portrayer_hip.h): per pixel the sum of its complete chunks, the sum of its open chunk and its count, row-major; the staging buffer the
// sampling kernel writes a launch's samples to (sized for the largest slice seen); device copies for the host-buffer paths; and the counts again on the host,
// so that an add that would take a pixel past 2^31 samples is refused before any HIP call.
struct pt_film {
    pt_context* ctx = nullptr;
    uint32_t width = 0, height = 0;
    PtBuf total, partial, count, staging, bg, out_rgb, out_linear;
    // pt_film_create_moments: the second moment per pixel. pt_film_add_map: the host map's device copy, the list of a launch round (its length in the
    // word in front of it), the plan's block sums. pt_film_error: the host path's device buffer.
    PtBuf q, budget, list, plan_work, out_err;
    // pt_film_denoise: the two work buffers of its levels (32 bytes per pixel each, allocated by the first denoise); the host path's device copies of the
    // guides and of the variance it returns.
    PtBuf dn_work[2], dn_position, dn_normal, dn_node, dn_albedo, out_var;  // (dn_albedo: pt_film_denoise_albedo's guide)
    bool moments = false;
    std::vector<uint32_t> counts;
};
static int pt_fail(pt_context* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}
#define PT_HIP(c, call)                                                                                   \
    do {                                                                                                  \
        hipError_t e_ = (call);                                                                           \
        if (e_ != hipSuccess) return pt_fail(c, PT_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

static int pt_reserve(pt_context* c, PtBuf& b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.bytes >= bytes) return PT_OK;
    if (b.p) { PT_HIP(c, hipFree(b.p)); b.p = nullptr; b.bytes = 0; }
    PT_HIP(c, hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    return PT_OK;
}
template <class T>
static int pt_upload(pt_context* c, PtBuf& b, const std::vector<T>& v) {
    int rc = pt_reserve(c, b, v.size() * sizeof(T));
    if (rc) return rc;
    if (!v.empty()) PT_HIP(c, hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return PT_OK;
}

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
// size has them (pt_render_common).
static int pt_pass_open(pt_context* c, PtPass& v, PtRenderArgs& r, uint32_t grid, bool frames, hipStream_t stream) {
    r.n_lanes = grid * PT_BLOCK;
    int rc;
    if ((rc = pt_reserve(c, v.stack_spill, (size_t)r.n_lanes * pt_stack_column(r.scene, r.stack_lds_cap) * 4))) return rc;
    if (frames && (rc = pt_reserve(c, v.spill, c->needs_spill ? (size_t)r.n_lanes * PT_SPILL_DEPTHS * PT_SPILL_STRIDE * sizeof(double) : 16))) return rc;
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
    bool two = !(c->have_scene && c->needs_spill);
    if (const char* e = getenv("PORTRAYER_TWO_STREAMS")) two = atoi(e) > 0;
    return (void*)c->slot[two ? (slot & 1) : 0].stream;
}
extern "C" int pt_context_next_slot(const pt_context* c) { return c ? c->slot_next : 0; }

// ------------------------------------------------------------------------------------------------
// Scene upload
// ------------------------------------------------------------------------------------------------
static void pt_transform_box(const double* m, const double lo[3], const double hi[3], PtBuildBox* out) {
    *out = pt_bvh_detail::empty_box();
    for (int ix = 0; ix < 2; ix++) for (int iy = 0; iy < 2; iy++) for (int iz = 0; iz < 2; iz++) {
        double x = ix ? hi[0] : lo[0], y = iy ? hi[1] : lo[1], z = iz ? hi[2] : lo[2];
        for (int r = 0; r < 3; r++) {
            double v = m[4 * r] * x + m[4 * r + 1] * y + m[4 * r + 2] * z + m[4 * r + 3];
            out->lo[r] = std::min(out->lo[r], v);
            out->hi[r] = std::max(out->hi[r], v);
        }
    }
}
static void pt_pad_box(PtBuildBox* b, double rel) {
    for (int k = 0; k < 3; k++) {
        double mag = std::max(std::fabs(b->lo[k]), std::fabs(b->hi[k]));
        double pad = rel * std::max(b->hi[k] - b->lo[k], mag) + 1e-300;
        b->lo[k] -= pad; b->hi[k] += pad;
    }
}

// ------------------------------------------------------------------------------------------------
// Steps of pt_scene_upload that pt_scene_update repeats for a moved scene: both call these, so a host-computed part of an updated
// scene is what an upload of the same scene computes.
// ------------------------------------------------------------------------------------------------
static void pt_pack_node_matrices(uint32_t n, const double* trans, const double* invtrans, const double* normal_trans, std::vector<double>& inv,
                                  std::vector<double>& fwd, std::vector<double>& nrm) {
    inv.resize(12 * (size_t)n); fwd.resize(12 * (size_t)n); nrm.resize(9 * (size_t)n);
    for (uint32_t i = 0; i < n; i++) {
        for (int r = 0; r < 12; r++) { inv[12 * (size_t)i + r] = invtrans[16 * (size_t)i + r]; fwd[12 * (size_t)i + r] = trans[16 * (size_t)i + r]; }
        for (int r = 0; r < 3; r++) for (int k = 0; k < 3; k++) nrm[9 * (size_t)i + 3 * r + k] = normal_trans[16 * (size_t)i + 4 * r + k];
    }
}

struct PtGraphArrays {
    std::vector<double> g_inv, g_fwd, g_nrm, own_inv;
    std::vector<uint32_t> hier_rec;
};
// PT_TRAVERSE_HIER: the graph nodes' matrices and, per flattened node, its path record and its own level's inverse. chain_off / chain are checked by the caller.
static void pt_pack_graph(uint32_t n, uint32_t g, const double* graph_trans, const double* graph_invtrans, const double* graph_normal_trans,
                          const std::vector<uint32_t>& chain_off, const std::vector<uint32_t>& chain, PtGraphArrays& out) {
    std::vector<double>&g_inv = out.g_inv, &g_fwd = out.g_fwd, &g_nrm = out.g_nrm, &own_inv = out.own_inv;
    std::vector<uint32_t>& hier_rec = out.hier_rec;
    g_inv.resize(12 * (size_t)g); g_fwd.resize(12 * (size_t)g); g_nrm.resize(9 * (size_t)g);
    for (uint32_t i = 0; i < g; i++) {
        for (int r = 0; r < 12; r++) { g_inv[12 * (size_t)i + r] = graph_invtrans[16 * (size_t)i + r]; g_fwd[12 * (size_t)i + r] = graph_trans[16 * (size_t)i + r]; }
        for (int r = 0; r < 3; r++) for (int k = 0; k < 3; k++) g_nrm[9 * (size_t)i + 3 * r + k] = graph_normal_trans[16 * (size_t)i + 4 * r + k];
    }
    // One record per flattened node for the walks (pt_node_local_ray_uniform): its path in one scalar fetch instead of three dependent
    // ones, and which of its levels are the identity (a group without a transform, like every reference scene's root): multiplying a
    // ray by such a level changes no bit unless a component is -0 or not finite, which the walk rules out once per ray.
    auto identity = [&](uint32_t gi) {
        for (int r = 0; r < 3; r++)
            for (int k = 0; k < 4; k++) {
                const double want = r == k ? 1.0 : 0.0;  // (== : a zero of either sign passes)
                if (g_inv[12 * (size_t)gi + 4 * r + k] != want || g_fwd[12 * (size_t)gi + 4 * r + k] != want) return false;
                if (k < 3 && g_nrm[9 * (size_t)gi + 3 * r + k] != want) return false;
            }
        return true;
    };
    std::vector<uint8_t> g_ident(g);
    for (uint32_t i = 0; i < g; i++) g_ident[i] = identity(i) ? 1 : 0;
    hier_rec.assign(8 * (size_t)n, 0u);
    own_inv.assign(12 * (size_t)n, 0.0);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t len = chain_off[i + 1] - chain_off[i];
        uint32_t* rec = &hier_rec[8 * (size_t)i];
        for (int r = 0; r < 12; r++) own_inv[12 * (size_t)i + r] = g_inv[12 * (size_t)chain[chain_off[i + 1] - 1] + r];  // the node's own level: the last of its path
        if (len > 7) { rec[0] = 255u; continue; }
        rec[0] = len;
        for (uint32_t k = 0; k < len; k++) {
            const uint32_t gi = chain[chain_off[i] + k];
            rec[1 + k] = gi;
            if (g_ident[gi]) rec[0] |= 1u << (8 + k);
        }
    }
}

// The box of a mesh's vertices and its largest extent (floored at 1e-30): triangle boxes are padded by 1e-7 ext, the mesh's own box by 1e-5 ext.
// pt_scene_upload and pt_scene_deform both call this.
static double pt_box_extent(const PtBuildBox& b) { return std::max(std::max(b.hi[0] - b.lo[0], b.hi[1] - b.lo[1]), std::max(b.hi[2] - b.lo[2], 1e-30)); }
static double pt_mesh_vertex_box(const double* pos, uint64_t n_verts, PtBuildBox* mb) {
    *mb = pt_bvh_detail::empty_box();
    for (uint64_t v = 0; v < n_verts; v++)
        for (int k = 0; k < 3; k++) { mb->lo[k] = std::min(mb->lo[k], pos[3 * v + k]); mb->hi[k] = std::max(mb->hi[k], pos[3 * v + k]); }
    return pt_box_extent(*mb);
}

// the padded model box of a stand-alone triangle (9 f64)
static void pt_triangle_model_box(const double* v, PtBuildBox* b) {
    double ext = 1e-30;
    for (int k = 0; k < 3; k++) {
        b->lo[k] = std::min(v[k], std::min(v[3 + k], v[6 + k])); b->hi[k] = std::max(v[k], std::max(v[3 + k], v[6 + k]));
        ext = std::max(ext, b->hi[k] - b->lo[k]);
    }
    for (int k = 0; k < 3; k++) { b->lo[k] -= 1e-6 * ext; b->hi[k] += 1e-6 * ext; }
}

// Conservative world-space boxes of the flattened nodes and their union, the scene tree's root box (c->root_lo / root_hi): every hit the
// primitive tests can accept lies inside its box (cube.rs:25 / plane.rs:31 accept points up to 1e-5 outside the unit shape; all shapes are
// padded by 1e-4 model units). Spheres, cylinders and cones get their exact boxes under the affine transform instead of the box of their
// transformed unit cube. `info`: 4 words per node (type, data, ..); pt_node_box_kernel (pt_build.hip) is the device's copy of the formulas.
static void pt_node_world_boxes(uint32_t n, const double* trans, const uint32_t* info, const std::vector<PtBuildBox>& mesh_box,
                                const std::vector<PtBuildBox>& tri_box, size_t mesh_tris, std::vector<PtBuildBox>& node_box, double root_lo[3], double root_hi[3]) {
    node_box.resize(n);
    for (uint32_t i = 0; i < n; i++) {
        const int t = (int)info[4 * (size_t)i];
        const uint32_t data = info[4 * (size_t)i + 1];
        const double* M = &trans[16 * (size_t)i];
        PtBuildBox& nb = node_box[i];
        auto disc = [&](double yc, double radius, PtBuildBox* b) {  // disc of `radius` in the model xz-plane at height yc
            for (int r = 0; r < 3; r++) {
                double c = M[4 * r + 1] * yc + M[4 * r + 3];
                double e = radius * std::sqrt(M[4 * r] * M[4 * r] + M[4 * r + 2] * M[4 * r + 2]);
                b->lo[r] = std::min(b->lo[r], c - e); b->hi[r] = std::max(b->hi[r], c + e);
            }
        };
        double lo[3], hi[3];
        bool boxed = false;
        switch (t) {
        case PT_PRIM_SPHERE:
            for (int r = 0; r < 3; r++) {
                double e = 1.0001 * std::sqrt(M[4 * r] * M[4 * r] + M[4 * r + 1] * M[4 * r + 1] + M[4 * r + 2] * M[4 * r + 2]);
                nb.lo[r] = M[4 * r + 3] - e; nb.hi[r] = M[4 * r + 3] + e;
            }
            boxed = true; break;
        case PT_PRIM_CYLINDER: nb = pt_bvh_detail::empty_box(); disc(0.5001, 0.5001, &nb); disc(-0.5001, 0.5001, &nb); boxed = true; break;
        case PT_PRIM_CONE: nb = pt_bvh_detail::empty_box(); disc(0.5001, 1e-4, &nb); disc(-0.5001, 0.5001, &nb); boxed = true; break;
        case PT_PRIM_PLANE: lo[0] = lo[2] = -0.5001; hi[0] = hi[2] = 0.5001; lo[1] = -1e-4; hi[1] = 1e-4; break;
        case PT_PRIM_MESH: case PT_PRIM_KDMESH: for (int k = 0; k < 3; k++) { lo[k] = mesh_box[data].lo[k]; hi[k] = mesh_box[data].hi[k]; } break;
        case PT_PRIM_TRIANGLE: for (int k = 0; k < 3; k++) { lo[k] = tri_box[data - mesh_tris].lo[k]; hi[k] = tri_box[data - mesh_tris].hi[k]; } break;
        default: lo[0] = lo[1] = lo[2] = -0.5001; hi[0] = hi[1] = hi[2] = 0.5001; break;  // cube
        }
        if (!boxed) pt_transform_box(M, lo, hi, &nb);
        pt_pad_box(&nb, 1e-9);
    }
    for (int k = 0; k < 3; k++) { root_lo[k] = INFINITY; root_hi[k] = -INFINITY; }
    for (uint32_t i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) { root_lo[k] = std::min(root_lo[k], node_box[i].lo[k]); root_hi[k] = std::max(root_hi[k], node_box[i].hi[k]); }
}

// The scene-level tree on the host: binned SAH over the nodes' world boxes (pt_bvh.h), built from index 0 and then moved to where it lives in the
// context's arrays: its nodes from `node_base` on in bvh, its leaf items (none when the leaves are direct) from `item_base` on in bvh_items.
static PtBvhRef pt_build_scene_tree(const std::vector<PtBuildBox>& node_box, int tlas_leaf, bool direct, size_t node_base, size_t item_base,
                                    std::vector<PtBvhNode>& nodes, std::vector<uint32_t>& items) {
    nodes.clear(); items.clear();
    PtBvhRef root = pt_bvh_build(node_box.data(), nullptr, node_box.size(), tlas_leaf, nodes, items, direct);
    auto moved = [&](uint32_t ref) -> uint32_t {
        if (ref == PT_REF_EMPTY) return ref;
        if (!(ref & PT_REF_LEAF)) return ref + (uint32_t)node_base;
        if (direct) return ref;
        return PT_REF_LEAF | (((((ref & ~PT_REF_LEAF) >> 3) + (uint32_t)item_base) << 3) | (ref & 7u));
    };
    for (PtBvhNode& nd : nodes) { nd.child0 = moved(nd.child0); nd.child1 = moved(nd.child1); }
    root.child = moved(root.child);
    return root;
}

// The reference's k-d tree over the flattened nodes (PT_TRAVERSE_KD) as the walks read it, with the conservative f32 boxes the culls use.
struct PtKdArrays {
    std::vector<PtKdNode> kdn;
    std::vector<uint32_t> kdi, kd_ref32;
    std::vector<float> node_box32, kd_box32;
    double kd_extent = 0.0;
    int kd_depth = 0, kd_levels = 0;
};
static int pt_pack_kd(pt_context* c, const pt_kdtree* kd, uint32_t n, const std::vector<PtBuildBox>& node_box, PtKdArrays& out) {
    std::vector<PtKdNode>& kdn = out.kdn;
    std::vector<uint32_t>&kdi = out.kdi, &kd_ref32 = out.kd_ref32;
    std::vector<float>&node_box32 = out.node_box32, &kd_box32 = out.kd_box32;
    int& kd_levels = out.kd_levels;  // split levels on the deepest path of the tree (root = level 0)
    if (kd->n_nodes == 0 || !kd->axis || !kd->plane || !kd->front || !kd->back || !kd->first || !kd->count || (kd->n_items && !kd->leaf_items))
        return pt_fail(c, PT_ERR_ARGUMENT, "incomplete k-d tree");
    kdn.resize(kd->n_nodes);
    for (uint32_t i = 0; i < kd->n_nodes; i++) {
        PtKdNode& k = kdn[i];
        k.axis = kd->axis[i]; k.plane = kd->plane[i]; k.front = kd->front[i]; k.back = kd->back[i];
        k.first = kd->first[i]; k.count = kd->count[i]; k.pad = 0; k.pad2[0] = k.pad2[1] = 0.0f; for (int r = 0; r < 6; r++) k.box[r] = 0.0f;
        if (k.axis >= 0) {
            if (k.axis > 2 || k.front < 0 || k.back < 0 || (uint32_t)k.front >= kd->n_nodes || (uint32_t)k.back >= kd->n_nodes)
                return pt_fail(c, PT_ERR_ARGUMENT, "k-d child out of range");
        } else if (k.first < 0 || k.count < 0 || (uint32_t)(k.first + k.count) > kd->n_items) {
            return pt_fail(c, PT_ERR_ARGUMENT, "k-d leaf range out of bounds");
        }
    }
    kdi.resize(kd->n_items);
    for (uint32_t i = 0; i < kd->n_items; i++) {
        if (kd->leaf_items[i] < 0 || (uint32_t)kd->leaf_items[i] >= n) return pt_fail(c, PT_ERR_ARGUMENT, "k-d leaf item out of range");
        kdi[i] = (uint32_t)kd->leaf_items[i];
    }
    double dx = kd->root_max[0] - kd->root_min[0], dy = kd->root_max[1] - kd->root_min[1], dz = kd->root_max[2] - kd->root_min[2];
    out.kd_extent = (dx * dx + dy * dy) + dz * dz;  // bounding_box.rs:95-99 magnitude_squared
    out.kd_depth = kd->max_depth < 0 ? 0 : kd->max_depth;
    node_box32.resize(6 * kdi.size());  // in leaf-item order: the walk reads a leaf's boxes one after the other
    for (size_t j = 0; j < kdi.size(); j++)
        for (int k = 0; k < 3; k++) {
            node_box32[6 * j + k] = pt_bvh_detail::round_down(node_box[kdi[j]].lo[k]);
            node_box32[6 * j + 3 + k] = pt_bvh_detail::round_up(node_box[kdi[j]].hi[k]);
        }
    // the wave-uniform k-d walk (pt_trace_packet_kd) reads a leaf reference and its cull box in ONE scalar fetch: 32 bytes {node, 0, box}
    kd_ref32.resize(8 * kdi.size());
    for (size_t j = 0; j < kdi.size(); j++) {
        kd_ref32[8 * j] = kdi[j]; kd_ref32[8 * j + 1] = 0u;
        memcpy(&kd_ref32[8 * j + 2], &node_box32[6 * j], 6 * sizeof(float));
    }
    {
        std::vector<std::pair<uint32_t, int>> todo;
        std::vector<uint8_t> seen(kdn.size(), 0);
        if (!kdn.empty()) todo.push_back({0u, 0});
        while (!todo.empty()) {
            auto [i, lev] = todo.back(); todo.pop_back();
            if (seen[i]) return pt_fail(c, PT_ERR_ARGUMENT, "k-d tree is not a tree");
            seen[i] = 1;
            if (kdn[i].axis < 0) continue;
            kd_levels = std::max(kd_levels, lev + 1);
            todo.push_back({(uint32_t)kdn[i].front, lev + 1}); todo.push_back({(uint32_t)kdn[i].back, lev + 1});
        }
    }
    if (kd_levels > PT_KD_WAVE_LEVELS)  // two bits of per-lane state per level in one 64-bit word (pt_trace_packet_kd); a tree that deep has > 2^32 leaves unless it is a degenerate chain
        return pt_fail(c, PT_ERR_SCENE, "k-d tree deeper than 32 levels (the limit of the k-d walk: include/portrayer_hip.h, pt_kdtree)");
    // what the walk's packed words can address: a stack entry is (node << 5) | level, a node is fetched at byte offset node << 6, a leaf reference at (first + i) << 5
    if (kdn.size() >= ((size_t)1 << 26)) return pt_fail(c, PT_ERR_SCENE, "k-d tree of 2^26 nodes or more");
    if (kd_ref32.size() / 8 >= ((size_t)1 << 27)) return pt_fail(c, PT_ERR_SCENE, "k-d tree with 2^27 leaf references or more");
    // children follow their parents in the linearised tree (pre-order): one backward sweep
    kd_box32.assign(6 * kdn.size(), 0.0f);
    for (size_t i = kdn.size(); i-- > 0;) {
        float* b = &kd_box32[6 * i];
        const PtKdNode& k = kdn[i];
        for (int r = 0; r < 3; r++) { b[r] = (float)PT_BOX_LIMIT; b[3 + r] = -(float)PT_BOX_LIMIT; }  // empty
        if (k.axis < 0) {
            for (int32_t j = 0; j < k.count; j++)
                for (int r = 0; r < 3; r++) {
                    b[r] = std::min(b[r], node_box32[6 * (size_t)(k.first + j) + r]);
                    b[3 + r] = std::max(b[3 + r], node_box32[6 * (size_t)(k.first + j) + 3 + r]);
                }
        } else if ((size_t)k.front > i && (size_t)k.back > i) {
            for (int r = 0; r < 3; r++) {
                b[r] = std::min(kd_box32[6 * (size_t)k.front + r], kd_box32[6 * (size_t)k.back + r]);
                b[3 + r] = std::max(kd_box32[6 * (size_t)k.front + 3 + r], kd_box32[6 * (size_t)k.back + 3 + r]);
            }
        } else {  // not in pre-order: no culling at this node
            for (int r = 0; r < 3; r++) { b[r] = -(float)PT_BOX_LIMIT; b[3 + r] = (float)PT_BOX_LIMIT; }
        }
    }
    for (size_t i = 0; i < kdn.size(); i++) for (int r = 0; r < 6; r++) kdn[i].box[r] = kd_box32[6 * i + r];
    return PT_OK;
}
// ... into the context's buffers and the view (k.kdn empty: another traversal)
static int pt_upload_kd(pt_context* c, const PtKdArrays& k, bool kd_mode) {
    int rc;
    if ((rc = pt_upload(c, c->node_box, k.node_box32)) || (rc = pt_upload(c, c->kd_box, k.kd_box32)) || (rc = pt_upload(c, c->kd, k.kdn)) ||
        (rc = pt_upload(c, c->kd_items, k.kdi)) || (rc = pt_upload(c, c->kd_ref, k.kd_ref32)))
        return rc;
    PtSceneView& v = c->view;
    v.kd = (const PtKdNode*)c->kd.p; v.kd_items = (const uint32_t*)c->kd_items.p;
    v.kd_extent = k.kd_extent;
    v.kd_ref = (const uint32_t*)c->kd_ref.p; v.kd_levels = k.kd_levels;
    v.node_box = kd_mode && !k.kdi.empty() ? (const float*)c->node_box.p : nullptr;
    v.kd_box = kd_mode ? (const float*)c->kd_box.p : nullptr;
    if (getenv("PORTRAYER_KD_NO_CULL")) v.kd_box = v.node_box = nullptr;  // experiment: the reference's walk as it is
    if (const char* e = getenv("PORTRAYER_KD_CULL")) { const int m = atoi(e); if (!(m & 1)) v.kd_box = nullptr; if (!(m & 2)) v.node_box = nullptr; }  // experiment: bit 0 tree nodes, bit 1 leaf references
    return PT_OK;
}

// fork / join of refracted subtrees (pt_shade.h) needs a recursion that draws no random numbers and a dielectric material to be of use
static void pt_set_light_flags(pt_context* c, const double* lights, uint32_t n_lights) {
    bool draws = c->res.mat_draws;
    for (uint32_t l = 0; l < n_lights; l++) {
        const double* L = &lights[15 * (size_t)l];
        const bool empty = (L[9] == 0.0 && L[10] == 0.0 && L[11] == 0.0) || (L[12] == 0.0 && L[13] == 0.0 && L[14] == 0.0);  // light.rs:51-53
        if (!empty) draws = true;
    }
    c->forkable = c->spawns && c->res.dielectric && !draws && n_lights <= PT_LIGHT_ROUND;
    c->one_ray = c->spawns && !c->res.dielectric;
}

// The walks' stack: a level of the four-child walk pushes up to three pending children; it covers two levels of the two-child tree in the plain
// collapse and at least one when nodes are opened by area. `tlas_depth`: of the scene-level tree (two-child form); `kd_depth`: of the k-d tree
// the scene is walked with NOW (PT_TRAVERSE_KD; it changes when nodes move).
static int pt_set_stack_cap(pt_context* c, int tlas_depth, int kd_depth) {
    const int collapse_mode = c->res.collapse_mode;
    auto wide = [&](int depth2) { return collapse_mode ? 3 * depth2 : 3 * ((depth2 + 1) / 2); };
    int cap = c->res.traverse == PT_TRAVERSE_KD ? 3 * (kd_depth + 1) + c->res.below + 2 : wide(tlas_depth) + c->res.below + 4;
    c->view.stack_cap = std::max(cap, 8);
    if (const char* e = getenv("PORTRAYER_STACK_CAP")) c->view.stack_cap = std::max(1, atoi(e));  // tests: force PT_ERR_TRAVERSAL
    if (c->view.stack_cap > 4096) return pt_fail(c, PT_ERR_SCENE, "tree too deep for the traversal stack");
    return PT_OK;
}

extern "C" int pt_scene_upload(pt_context* c, const pt_scene* s, int traverse, const pt_kdtree* kd) {
    if (!c || !s) return PT_ERR_ARGUMENT;
    if (traverse != PT_TRAVERSE_FLAT && traverse != PT_TRAVERSE_KD && traverse != PT_TRAVERSE_HIER)
        return pt_fail(c, PT_ERR_ARGUMENT, "traverse must be PT_TRAVERSE_FLAT, PT_TRAVERSE_KD or PT_TRAVERSE_HIER");
    if (traverse == PT_TRAVERSE_HIER && s->n_nodes &&
        (!s->n_graph_nodes || !s->graph_trans || !s->graph_invtrans || !s->graph_normal_trans || !s->node_chain_off || !s->node_chain || !s->node_dfs_rank))
        return pt_fail(c, PT_ERR_ARGUMENT, "PT_TRAVERSE_HIER needs the scene graph (graph_*, node_chain*, node_dfs_rank)");
    if (traverse == PT_TRAVERSE_KD && !kd) return pt_fail(c, PT_ERR_ARGUMENT, "PT_TRAVERSE_KD needs the host-built k-d tree");
    if (s->n_nodes && (!s->trans || !s->invtrans || !s->normal_trans || !s->prim_type || !s->prim_data || !s->prim_flags || !s->material))
        return pt_fail(c, PT_ERR_ARGUMENT, "null node array");
    PT_HIP(c, hipSetDevice(c->device));
    c->have_scene = false;
    const uint32_t n = s->n_nodes;
    const bool verbose = getenv("PORTRAYER_VERBOSE") != nullptr;
    auto t_begin = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!verbose) return;
        auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[pt_scene_upload] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t_begin).count());
        t_begin = now;
    };

    // ---- triangles: every mesh expanded to 72-byte vertex records, stand-alone triangles appended
    std::vector<uint64_t> tri_first(s->n_meshes + 1, 0);
    size_t mesh_tris = s->n_meshes ? (size_t)s->mesh_tri_off[s->n_meshes] : 0;
    size_t total_tris = mesh_tris + s->n_triangles;
    bool any_normals = false;
    for (uint32_t i = 0; i < n; i++) {
        int t = s->prim_type[i];
        if (t < PT_PRIM_SPHERE || t > PT_PRIM_CONE) return pt_fail(c, PT_ERR_ARGUMENT, "unknown primitive type");
        if (s->material[i] < 0 || (uint32_t)s->material[i] >= s->n_materials) return pt_fail(c, PT_ERR_ARGUMENT, "material index out of range");
        if (t == PT_PRIM_MESH || t == PT_PRIM_KDMESH) {
            if (s->prim_data[i] < 0 || (uint32_t)s->prim_data[i] >= s->n_meshes) return pt_fail(c, PT_ERR_ARGUMENT, "mesh index out of range");
            if (s->prim_flags[i] & 1) {
                if (!s->mesh_has_normals || !s->mesh_has_normals[s->prim_data[i]] || !s->mesh_normals)
                    return pt_fail(c, PT_ERR_SCENE, "smooth shading needs a vertex normal per vertex (mesh.rs:135-138)");
                any_normals = true;
            }
        } else if (t == PT_PRIM_TRIANGLE) {
            if (s->prim_data[i] < 0 || (uint32_t)s->prim_data[i] >= s->n_triangles) return pt_fail(c, PT_ERR_ARGUMENT, "triangle index out of range");
            if (s->prim_flags[i] & 1) { if (!s->tri_normals) return pt_fail(c, PT_ERR_SCENE, "triangle normals missing"); any_normals = true; }
        }
    }
    std::vector<double> tri_v(total_tris * 9), tri_n(any_normals ? total_tris * 9 : 0);
    std::vector<PtMeshInfo> meshes(s->n_meshes);
    std::vector<PtBvhNode> bvh;
    std::vector<uint32_t> items;
    std::vector<PtBuildBox> mesh_box(s->n_meshes);
    int max_blas_depth = 0;
    int collapse_mode = 1;  // how two-child trees become four-child trees (pt_collapse4_kernel): 0 grandchildren, 1 mesh trees opened by area, 2 every tree by area
    int blas_leaf = 2;  // triangles per mesh-tree leaf (measured: 2 beats 1, 3 and 4 by 2-5 % on cows / big-soup)
    if (const char* e = getenv("PORTRAYER_BLAS_LEAF")) blas_leaf = std::min(std::max(1, atoi(e)), 8);
    // Where a mesh's triangle tree is built: on the host (binned SAH, pt_bvh.h: the better tree) or on the
    // device (Morton-order tree, pt_build.h: ~100x faster to build). PORTRAYER_BUILD = host | device | auto;
    // auto takes the device for meshes of PORTRAYER_BUILD_MIN (default 65536) triangles or more.
    int build_mode = 2;
    size_t device_build_min = 65536;
    if (const char* e = getenv("PORTRAYER_BUILD")) build_mode = !strcmp(e, "host") ? 0 : (!strcmp(e, "device") ? 1 : 2);
    if (const char* e = getenv("PORTRAYER_BUILD_MIN")) device_build_min = (size_t)std::max(16, atoi(e));
    struct DeviceMesh { uint32_t m, t0, count; double lo[3], hi[3], pad; };
    std::vector<DeviceMesh> device_meshes;
    std::vector<pt_context::Resident::MeshPlace> place(s->n_meshes);
    for (uint32_t m = 0; m < s->n_meshes; m++) {
        uint64_t v0 = s->mesh_vert_off[m], v1 = s->mesh_vert_off[m + 1], t0 = s->mesh_tri_off[m], t1 = s->mesh_tri_off[m + 1];
        if (v1 <= v0) return pt_fail(c, PT_ERR_SCENE, "meshes must have at least one vertex (mesh.rs:71)");
        const double* pos = s->mesh_positions + 3 * v0;
        const double* nrm = (s->mesh_normals && s->mesh_has_normals && s->mesh_has_normals[m]) ? s->mesh_normals + 3 * v0 : nullptr;
        PtBuildBox mb;
        const double ext = pt_mesh_vertex_box(pos, v1 - v0, &mb);
        const bool on_device = (build_mode == 1 && t1 - t0 >= 16) || (build_mode == 2 && t1 - t0 >= device_build_min);
        std::vector<PtBuildBox> boxes(on_device ? 0 : t1 - t0);
        std::vector<uint32_t> ids(on_device ? 0 : t1 - t0);
        for (uint64_t t = t0; t < t1; t++) {
            PtBuildBox b = pt_bvh_detail::empty_box();
            for (int corner = 0; corner < 3; corner++) {
                uint32_t vi = s->mesh_indices[3 * t + corner];
                if (vi >= v1 - v0) return pt_fail(c, PT_ERR_ARGUMENT, "mesh index out of range");
                for (int k = 0; k < 3; k++) {
                    double x = pos[3 * (size_t)vi + k];
                    tri_v[9 * t + 3 * corner + k] = x;
                    if (any_normals) tri_n[9 * t + 3 * corner + k] = nrm ? nrm[3 * (size_t)vi + k] : 0.0;
                    b.lo[k] = std::min(b.lo[k], x); b.hi[k] = std::max(b.hi[k], x);
                }
            }
            if (on_device) continue;
            for (int k = 0; k < 3; k++) { b.lo[k] -= 1e-7 * ext; b.hi[k] += 1e-7 * ext; }
            boxes[t - t0] = b;
            ids[t - t0] = (uint32_t)t;
        }
        PtBvhRef ref;
        ref.child = PT_REF_EMPTY; ref.depth = 0;
        pt_context::Resident::MeshPlace& pl = place[m];
        pl.n_verts = (uint32_t)(v1 - v0); pl.has_normals = nrm != nullptr; pl.device_built = on_device;
        pl.node_first = (uint32_t)bvh.size(); pl.item_first = (uint32_t)items.size();
        if (on_device) {  // built after the triangles are in HBM (below); the root is filled in then
            DeviceMesh dm;
            dm.m = m; dm.t0 = (uint32_t)t0; dm.count = (uint32_t)(t1 - t0);
            for (int k = 0; k < 3; k++) { dm.lo[k] = mb.lo[k]; dm.hi[k] = mb.hi[k]; }
            dm.pad = 1e-7 * ext;
            device_meshes.push_back(dm);
        } else {
            ref = pt_bvh_build(boxes.data(), ids.data(), boxes.size(), blas_leaf, bvh, items);
            pl.node_count = (uint32_t)bvh.size() - pl.node_first; pl.item_count = (uint32_t)items.size() - pl.item_first; pl.depth = ref.depth;
        }
        max_blas_depth = std::max(max_blas_depth, ref.depth);
        PtMeshInfo& mi = meshes[m];
        for (int r = 0; r < 12; r++) mi.bbox_inv[r] = s->mesh_bounds_invtrans ? s->mesh_bounds_invtrans[16 * (size_t)m + r] : 0.0;
        if (!s->mesh_bounds_invtrans) return pt_fail(c, PT_ERR_ARGUMENT, "mesh_bounds_invtrans missing");
        mi.tri_first = (uint32_t)t0; mi.tri_count = (uint32_t)(t1 - t0);
        mi.blas_root = ref.child; mi.kd_root = -1; mi.kd_extent = 0.0;
        for (int r = 0; r < 12; r++) mi.kd_bbox_inv[r] = 0.0;
        for (int k = 0; k < 3; k++) { mb.lo[k] -= 1e-5 * ext; mb.hi[k] += 1e-5 * ext; }
        mesh_box[m] = mb;
    }
    lap("triangles + mesh trees");
    // ---- KDMesh triangle trees (reference structure)
    std::vector<PtKdNode> mkd;
    std::vector<uint32_t> mkd_items;
    std::vector<float> mkd_box, mkd_item_box;  // conservative f32 bounds per KDMesh tree node / per leaf reference (pt_kdmesh_hit's culls)
    int max_kdm_depth = 0;
    bool any_kdmesh = false;
    if (s->mesh_kd_root && s->n_kdm_nodes) {
        if (!s->kdm_axis || !s->kdm_plane || !s->kdm_front || !s->kdm_back || !s->kdm_first || !s->kdm_count || (s->n_kdm_items && !s->kdm_items) ||
            !s->mesh_kd_bounds || !s->mesh_kd_bounds_invtrans)
            return pt_fail(c, PT_ERR_ARGUMENT, "incomplete KDMesh tree arrays");
        mkd.resize(s->n_kdm_nodes);
        for (uint32_t i = 0; i < s->n_kdm_nodes; i++) {
            PtKdNode& k = mkd[i];
            k.axis = s->kdm_axis[i]; k.plane = s->kdm_plane[i]; k.front = s->kdm_front[i]; k.back = s->kdm_back[i];
            k.first = s->kdm_first[i]; k.count = s->kdm_count[i]; k.pad = 0; k.pad2[0] = k.pad2[1] = 0.0f; for (int r = 0; r < 6; r++) k.box[r] = 0.0f;
            if (k.axis >= 0) {
                if (k.axis > 2 || k.front < 0 || k.back < 0 || (uint32_t)k.front >= s->n_kdm_nodes || (uint32_t)k.back >= s->n_kdm_nodes)
                    return pt_fail(c, PT_ERR_ARGUMENT, "KDMesh tree child out of range");
            } else if (k.first < 0 || k.count < 0 || (uint32_t)(k.first + k.count) > s->n_kdm_items) {
                return pt_fail(c, PT_ERR_ARGUMENT, "KDMesh leaf range out of bounds");
            }
        }
        mkd_items.assign(s->n_kdm_items, 0);
        mkd_box.assign(6 * (size_t)s->n_kdm_nodes, 0.0f);
        mkd_item_box.assign(6 * (size_t)s->n_kdm_items, 0.0f);
        // leaf items are local triangle indices: make them global, mesh by mesh (a leaf belongs to the mesh whose tree reaches it)
        std::vector<int32_t> owner(s->n_kdm_nodes, -1);
        for (uint32_t m = 0; m < s->n_meshes; m++) {
            int32_t root = s->mesh_kd_root[m];
            if (root < 0) continue;
            if ((uint32_t)root >= s->n_kdm_nodes) return pt_fail(c, PT_ERR_ARGUMENT, "KDMesh root out of range");
            std::vector<int32_t> todo{root}, visited;
            const double tri_pad = 1e-7 * std::max(std::max(mesh_box[m].hi[0] - mesh_box[m].lo[0], mesh_box[m].hi[1] - mesh_box[m].lo[1]),
                                                   std::max(mesh_box[m].hi[2] - mesh_box[m].lo[2], 1e-30));
            while (!todo.empty()) {
                int32_t i = todo.back(); todo.pop_back();
                if (owner[i] >= 0) return pt_fail(c, PT_ERR_ARGUMENT, "KDMesh trees must not share nodes");
                owner[i] = (int32_t)m;
                visited.push_back(i);
                if (mkd[i].axis >= 0) { todo.push_back(mkd[i].front); todo.push_back(mkd[i].back); }
                else for (int32_t k = 0; k < mkd[i].count; k++) {
                    int32_t local = s->kdm_items[mkd[i].first + k];
                    if (local < 0 || (uint64_t)local >= s->mesh_tri_off[m + 1] - s->mesh_tri_off[m]) return pt_fail(c, PT_ERR_ARGUMENT, "KDMesh leaf triangle out of range");
                    const uint64_t g = s->mesh_tri_off[m] + (uint64_t)local;
                    mkd_items[mkd[i].first + k] = (uint32_t)g;
                    float* ib = &mkd_item_box[6 * (size_t)(mkd[i].first + k)];  // the triangle's padded box, for the walk's pre-cull
                    for (int r = 0; r < 3; r++) {
                        const double* v = &tri_v[9 * g];
                        ib[r] = pt_bvh_detail::round_down(std::min(v[r], std::min(v[3 + r], v[6 + r])) - tri_pad);
                        ib[3 + r] = pt_bvh_detail::round_up(std::max(v[r], std::max(v[3 + r], v[6 + r])) + tri_pad);
                    }
                }
            }
            for (size_t vi = visited.size(); vi-- > 0;) {  // children were discovered after their parents: bounds bottom-up
                const int32_t i = visited[vi];
                float* b = &mkd_box[6 * (size_t)i];
                for (int r = 0; r < 3; r++) { b[r] = (float)PT_BOX_LIMIT; b[3 + r] = -(float)PT_BOX_LIMIT; }
                auto grow = [&](const float* o) { for (int r = 0; r < 3; r++) { b[r] = std::min(b[r], o[r]); b[3 + r] = std::max(b[3 + r], o[3 + r]); } };
                if (mkd[i].axis >= 0) { grow(&mkd_box[6 * (size_t)mkd[i].front]); grow(&mkd_box[6 * (size_t)mkd[i].back]); }
                else for (int32_t k = 0; k < mkd[i].count; k++) grow(&mkd_item_box[6 * (size_t)(mkd[i].first + k)]);
            }
            PtMeshInfo& mi = meshes[m];
            mi.kd_root = root;
            any_kdmesh = true;
            const double* b = s->mesh_kd_bounds + 6 * (size_t)m;
            double dx = b[3] - b[0], dy = b[4] - b[1], dz = b[5] - b[2];
            mi.kd_extent = (dx * dx + dy * dy) + dz * dz;  // bounding_box.rs:95-99
            for (int r = 0; r < 12; r++) mi.kd_bbox_inv[r] = s->mesh_kd_bounds_invtrans[16 * (size_t)m + r];
            max_kdm_depth = std::max(max_kdm_depth, s->mesh_kd_depth ? std::max(s->mesh_kd_depth[m], 0) : 24);
        }
    }
    for (uint32_t t = 0; t < s->n_triangles; t++)
        for (int k = 0; k < 9; k++) {
            tri_v[9 * (mesh_tris + t) + k] = s->tri_vertices[9 * (size_t)t + k];
            if (any_normals) tri_n[9 * (mesh_tris + t) + k] = s->tri_normals ? s->tri_normals[9 * (size_t)t + k] : 0.0;
        }

    // ---- nodes
    std::vector<double> inv, fwd, nrm;
    std::vector<uint32_t> info(4 * (size_t)n);
    PtGraphArrays graph;
    std::vector<uint32_t> chain_off, chain, dfs_rank;
    if (traverse == PT_TRAVERSE_HIER && n) {
        const uint32_t g = s->n_graph_nodes;
        chain_off.assign(s->node_chain_off, s->node_chain_off + n + 1);
        if (chain_off[0] != 0) return pt_fail(c, PT_ERR_ARGUMENT, "node_chain_off must start at 0");
        for (uint32_t i = 0; i < n; i++)
            if (chain_off[i + 1] <= chain_off[i]) return pt_fail(c, PT_ERR_ARGUMENT, "every flattened node needs a non-empty path (it contains at least itself)");
        chain.assign(s->node_chain, s->node_chain + chain_off[n]);
        for (uint32_t id : chain) if (id >= g) return pt_fail(c, PT_ERR_ARGUMENT, "node_chain names a graph node out of range");
        dfs_rank.assign(s->node_dfs_rank, s->node_dfs_rank + n);
        pt_pack_graph(n, g, s->graph_trans, s->graph_invtrans, s->graph_normal_trans, chain_off, chain, graph);
    }
    pt_pack_node_matrices(n, s->trans, s->invtrans, s->normal_trans, inv, fwd, nrm);
    std::vector<PtBuildBox> tri_box(s->n_triangles);
    for (uint32_t t = 0; t < s->n_triangles; t++) pt_triangle_model_box(&tri_v[9 * (mesh_tris + t)], &tri_box[t]);
    for (uint32_t i = 0; i < n; i++) {
        int t = s->prim_type[i];
        uint32_t data = (uint32_t)s->prim_data[i];
        if (t == PT_PRIM_TRIANGLE) data = (uint32_t)(mesh_tris + data);
        info[4 * (size_t)i] = (uint32_t)t; info[4 * (size_t)i + 1] = data;
        info[4 * (size_t)i + 2] = (uint32_t)s->prim_flags[i]; info[4 * (size_t)i + 3] = (uint32_t)s->material[i];
    }
    std::vector<PtBuildBox> node_box;
    pt_node_world_boxes(n, s->trans, info.data(), mesh_box, tri_box, mesh_tris, node_box, c->root_lo, c->root_hi);
    int tlas_leaf = 1;  // primitive tests (f64, ~200 instructions) cost far more than a node visit: measured best on big-scene
    if (const char* e = getenv("PORTRAYER_TLAS_LEAF")) tlas_leaf = std::max(1, atoi(e));
    const bool tlas_direct = tlas_leaf == 1 && n < (1u << 28);
    // the scene-level tree keeps room for the n - 1 nodes any tree over n leaves can have: pt_scene_update builds its trees into the same place
    const size_t tlas_first = bvh.size(), tlas_items = items.size(), tlas_cap = n ? n - 1 : 0;
    PtBvhRef tlas;
    {
        std::vector<PtBvhNode> tl_nodes;
        std::vector<uint32_t> tl_items;
        tlas = pt_build_scene_tree(node_box, tlas_leaf, tlas_direct, tlas_first, tlas_items, tl_nodes, tl_items);
        bvh.insert(bvh.end(), tl_nodes.begin(), tl_nodes.end());
        items.insert(items.end(), tl_items.begin(), tl_items.end());
        PtBvhNode unused;
        memset(&unused, 0, sizeof unused);
        unused.child0 = unused.child1 = PT_REF_EMPTY;
        bvh.resize(tlas_first + tlas_cap, unused);
    }
    const size_t tlas_end = bvh.size();

    // ---- k-d tree (reference structure, KD mode)
    PtKdArrays kda;
    int rc;
    if (traverse == PT_TRAVERSE_KD && (rc = pt_pack_kd(c, kd, n, node_box, kda))) return rc;
    lap("scene tree");
    if ((rc = pt_upload(c, c->tri_v, tri_v))) return rc;
    {   // the edge form of every triangle (pt_triangle_hit_e): corner a, a - b, a - c
        std::vector<double> tri_e(tri_v.size());
        for (size_t t = 0; t < total_tris; t++) {
            const double* v = &tri_v[9 * t];
            double* e = &tri_e[9 * t];
            e[0] = v[0]; e[1] = v[1]; e[2] = v[2];
            e[3] = v[0] - v[3]; e[4] = v[1] - v[4]; e[5] = v[2] - v[5];
            e[6] = v[0] - v[6]; e[7] = v[1] - v[7]; e[8] = v[2] - v[8];
        }
        if ((rc = pt_upload(c, c->tri_e, tri_e))) return rc;
    }
    size_t tree_nodes = 0;
    {   // tree arrays: the host-built part first, then room for the device-built mesh trees
        size_t n_nodes = bvh.size(), n_items = items.size();
        for (const DeviceMesh& dm : device_meshes) { n_nodes += PT_DEVICE_TREE_NODES(dm.count); n_items += PT_DEVICE_TREE_ITEMS(dm.count, blas_leaf); }
        if (n_items >= (1u << 28) || n_nodes >= (1u << 26)) return pt_fail(c, PT_ERR_SCENE, "too many triangles for the 32-bit tree references (a node is addressed by a 32-bit byte offset: 2^26 nodes)");
        if ((rc = pt_reserve(c, c->bvh, n_nodes * sizeof(PtBvhNode))) || (rc = pt_reserve(c, c->bvh_items, n_items * sizeof(uint32_t)))) return rc;
        if (!bvh.empty()) PT_HIP(c, hipMemcpy(c->bvh.p, bvh.data(), bvh.size() * sizeof(PtBvhNode), hipMemcpyHostToDevice));
        if (!items.empty()) PT_HIP(c, hipMemcpy(c->bvh_items.p, items.data(), items.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        lap("upload triangles + host trees");
        uint32_t node_base = (uint32_t)bvh.size(), item_base = (uint32_t)items.size();
        float device_ms = 0.0f;
        int rounds = 0;
        for (const DeviceMesh& dm : device_meshes) {
            PtDeviceBuildResult res;
            pt_context::Resident::MeshPlace& pl = place[dm.m];
            pl.node_first = node_base; pl.node_count = PT_DEVICE_TREE_NODES(dm.count); pl.item_first = item_base; pl.item_count = PT_DEVICE_TREE_ITEMS(dm.count, blas_leaf);
            // entries of the place that the tree will not use name no children (pt_device_tree_parents reads the whole range)
            PT_HIP(c, hipMemset((PtBvhNode*)c->bvh.p + node_base, 0xFF, (size_t)pl.node_count * sizeof(PtBvhNode)));
            PT_HIP(c, pt_device_build_mesh_tree((const double*)c->tri_v.p, dm.t0, dm.count, dm.lo, dm.hi, dm.pad, blas_leaf, (PtBvhNode*)c->bvh.p, node_base,
                                                (uint32_t*)c->bvh_items.p, item_base, nullptr, &res));
            meshes[dm.m].blas_root = res.root;
            max_blas_depth = std::max(max_blas_depth, res.depth);
            pl.depth = res.depth;
            node_base += PT_DEVICE_TREE_NODES(dm.count); item_base += PT_DEVICE_TREE_ITEMS(dm.count, blas_leaf);
            device_ms += res.ms; rounds += res.rounds;
        }
        if (verbose && !device_meshes.empty()) fprintf(stderr, "[pt_scene_upload] device tree build: %zu mesh(es), %.2f ms, %d clustering rounds, depth %d\n", device_meshes.size(), device_ms, rounds, max_blas_depth);
        lap("device mesh trees");
        // the walks read the four-child form of every tree (scene tree and mesh trees alike)
        if (const char* e = getenv("PORTRAYER_COLLAPSE")) collapse_mode = strcmp(e, "plain") == 0 ? 0 : (strcmp(e, "area") == 0 ? 2 : 1);
        if ((rc = pt_reserve(c, c->bvh4, std::max<size_t>(n_nodes, 1) * sizeof(PtBvh4Node)))) return rc;
        if (n_nodes) {
            hipLaunchKernelGGL(pt_collapse4_kernel, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, nullptr, (const PtBvhNode*)c->bvh.p, (PtBvh4Node*)c->bvh4.p, (uint32_t)n_nodes, collapse_mode, (uint32_t)tlas_first, (uint32_t)tlas_end, 0u, (uint32_t)n_nodes);
            PT_HIP(c, hipGetLastError());
            PT_HIP(c, hipDeviceSynchronize());
        }
        tree_nodes = n_nodes;
        lap("four-child form");
        if ((rc = pt_reserve(c, c->tri_leaf, std::max<size_t>(n_items, 1) * 80))) return rc;
        if (n_items && total_tris) {
            hipLaunchKernelGGL(pt_tri_leaf_kernel, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, nullptr, (const uint32_t*)c->bvh_items.p, (uint32_t)n_items, (const double*)c->tri_e.p,
                               (uint32_t)total_tris, (double*)c->tri_leaf.p);
            PT_HIP(c, hipGetLastError());
            PT_HIP(c, hipDeviceSynchronize());
        }
        lap("triangle records in leaf order");
    }
    for (size_t i = 0; i < mkd.size() && !mkd_box.empty(); i++) for (int r = 0; r < 6; r++) mkd[i].box[r] = mkd_box[6 * i + r];
    if ((rc = pt_upload(c, c->g_inv, graph.g_inv)) || (rc = pt_upload(c, c->g_fwd, graph.g_fwd)) || (rc = pt_upload(c, c->g_nrm, graph.g_nrm)) ||
        (rc = pt_upload(c, c->chain_off, chain_off)) || (rc = pt_upload(c, c->chain, chain)) || (rc = pt_upload(c, c->dfs_rank, dfs_rank)) ||
        (rc = pt_upload(c, c->hier_rec, graph.hier_rec)) || (rc = pt_upload(c, c->own_inv, graph.own_inv)))
        return rc;
    if ((rc = pt_upload(c, c->inv, inv)) || (rc = pt_upload(c, c->fwd, fwd)) || (rc = pt_upload(c, c->nrm, nrm)) ||
        (rc = pt_upload(c, c->info, info)) || (rc = pt_upload(c, c->tri_n, tri_n)) ||
        (rc = pt_upload(c, c->meshes, meshes)) || (rc = pt_upload(c, c->mkd, mkd)) ||
        (rc = pt_upload(c, c->mkd_items, mkd_items)) || (rc = pt_upload(c, c->mkd_box, mkd_box)) || (rc = pt_upload(c, c->mkd_item_box, mkd_item_box)))
        return rc;
    std::vector<double> mats(s->materials, s->materials + 10 * (size_t)s->n_materials);
    c->needs_spill = s->n_lights > PT_LIGHT_ROUND;
    c->spawns = false;
    for (uint32_t m = 0; m < s->n_materials; m++) if (mats[10 * (size_t)m + 7] > 0.0) c->needs_spill = c->spawns = true;  // material.rs:216: reflectivity > 0 spawns children
    // The 4-waves-per-SIMD kernel for scenes where the tree walk outweighs the shading: many scene-level nodes or many instanced
    // triangles, nothing reflective, flat_scene semantics (measured: big-scene +8.7 %, big-soup +6.8 %; macho-cows
    // with its 23 nodes and 17,500 triangles -8 %; reflective scenes and the k-d walk lose, profiles/r02/notes.md)
    {
        uint64_t instanced_tris = 0;
        for (uint32_t i = 0; i < n; i++)
            if (s->prim_type[i] == PT_PRIM_MESH || s->prim_type[i] == PT_PRIM_KDMESH) instanced_tris += s->mesh_tri_off[s->prim_data[i] + 1] - s->mesh_tri_off[s->prim_data[i]];
        // hierarchical semantics (round 3, straight-line kernel): mesh-free scenes with many nodes gain like flat_scene ones (big-scene 25.7 ->
        // 29.4 Gray/s at 4 waves); with mesh instances the walk carries a second ray and spills at 128 registers (macho-cows 16.4 -> 12.0) unless
        // the triangle trees dominate (the 1.25 M-triangle soup: equal)
        // Since the register work of round 3 (arguments re-read, colour parked in LDS, an instantiation of the hierarchical semantics without
        // the KDMesh walker) scenes with plain Mesh instances of any size gain too (c41: macho-cows 21.4 -> 23.4 Gray/s, hierarchical 18.7 -> 19.7);
        // with KDMesh trees the kernels still spill 100+ registers at 128 and stay at 3 waves unless the triangle trees dominate.
        const bool plain_meshes = s->n_meshes > 0 && !any_kdmesh;
        c->four_waves = !c->spawns && ((traverse == PT_TRAVERSE_FLAT && (n >= 256 || instanced_tris >= 65536)) ||
                                       (traverse == PT_TRAVERSE_HIER && ((s->n_meshes == 0 && n >= 256) || instanced_tris >= 65536)));
        c->four_waves_untextured = !c->spawns && plain_meshes && (traverse == PT_TRAVERSE_FLAT || traverse == PT_TRAVERSE_HIER);  // (textured: flat_scene loses 10 % at 4 waves, c45)
        // The hierarchical semantics without KDMesh trees gain at 4 waves whatever the scene (their leaf tests wait for a path record and a matrix per
        // level): macho-cows +5 %, fish (textured) +5 %, normal-mapping (11 textured primitives) +12 %, the mirror scene's chain kernel +9 % (c41, c45).
        c->four_waves_hier = !c->spawns && traverse == PT_TRAVERSE_HIER && !any_kdmesh;
        // mesh-free scenes go one further: 5 waves per SIMD (96 registers, 17 of the kernel's spilled; big-scene 34.4 -> 37.0, hierarchical
        // 29.4 -> 32.5 Gray/s; the k-d walk, 50 spilled, loses and stays at 4)
        c->five_waves = c->four_waves && s->n_meshes == 0 && traverse != PT_TRAVERSE_KD;
        // ... and so do scenes of very many triangles in plain Mesh instances (round 4, c29: their walks wait for node fetches - 3 -> 4 waves was +18 % -; the 1.25 M-triangle
        // scenes +3.7 % / +3.2 %, hierarchical +2.6 %, at 96 registers with 57 spilled; macho-cows, 17,500 triangles, loses 15 % and stays at 4)
        // Round 5 (c47 / c48, after the tree step and the instance walk issue fewer scalar instructions): flat_scene is now FASTER at 4 waves (big-soup 18.96 -> 18.75 ms,
        // big-mesh 19.16 -> 18.86; 18 spilled registers instead of 69) and takes 4; the hierarchical semantics still gain 1 % at 5 and keep them.
        c->five_waves_mesh = !c->spawns && plain_meshes && instanced_tris >= 65536 && traverse == PT_TRAVERSE_HIER;
    }
    std::vector<double> lights(s->lights, s->lights + 15 * (size_t)s->n_lights);
    {   // what the materials say about the recursion; the lights have their say in pt_set_light_flags
        bool draws = false, dielectric = false;
        for (uint32_t m = 0; m < s->n_materials; m++) {
            if (mats[10 * (size_t)m + 7] > 0.0 && mats[10 * (size_t)m + 8] > 0.0) draws = true;   // glossy reflection (material.rs:221-239)
            if (mats[10 * (size_t)m + 7] > 0.0 && mats[10 * (size_t)m + 9] > 0.0) dielectric = true;
        }
        c->res.mat_draws = draws; c->res.dielectric = dielectric;
        pt_set_light_flags(c, lights.data(), s->n_lights);
    }
    if ((rc = pt_upload(c, c->materials, mats)) || (rc = pt_upload(c, c->lights, lights))) return rc;

    // ---- textures / normal maps (texture.rs)
    bool textured = false;
    for (uint32_t m = 0; m < s->n_materials; m++)
        if ((s->material_texture && s->material_texture[m] >= 0) || (s->material_normal_map && s->material_normal_map[m] >= 0)) textured = true;
    std::vector<int32_t> mat_maps;
    std::vector<double> uv_trans, srgb_lut, tri_uv;
    std::vector<PtTexInfo> texinfo;
    std::vector<uint8_t> tex_rgb;
    if (textured) {
        if (s->n_textures == 0 || !s->texture_size || !s->texture_offset || !s->texture_rgb) return pt_fail(c, PT_ERR_ARGUMENT, "textured material without texture data");
        size_t tex_bytes = 0;
        texinfo.resize(s->n_textures);
        for (uint32_t t = 0; t < s->n_textures; t++) {
            texinfo[t].offset = s->texture_offset[t]; texinfo[t].width = s->texture_size[2 * t]; texinfo[t].height = s->texture_size[2 * t + 1];
            if (texinfo[t].width == 0 || texinfo[t].height == 0) return pt_fail(c, PT_ERR_ARGUMENT, "empty texture");
            tex_bytes = std::max(tex_bytes, (size_t)texinfo[t].offset + 3 * (size_t)texinfo[t].width * texinfo[t].height);
        }
        tex_rgb.assign(s->texture_rgb, s->texture_rgb + tex_bytes);
        mat_maps.resize(2 * (size_t)s->n_materials);
        uv_trans.resize(9 * (size_t)s->n_materials);
        for (uint32_t m = 0; m < s->n_materials; m++) {
            int32_t a = s->material_texture ? s->material_texture[m] : -1, b = s->material_normal_map ? s->material_normal_map[m] : -1;
            if (a >= (int32_t)s->n_textures || b >= (int32_t)s->n_textures) return pt_fail(c, PT_ERR_ARGUMENT, "texture index out of range");
            mat_maps[2 * m] = a < 0 ? -1 : a; mat_maps[2 * m + 1] = b < 0 ? -1 : b;
            for (int k = 0; k < 9; k++) uv_trans[9 * (size_t)m + k] = s->material_uv_trans ? s->material_uv_trans[9 * (size_t)m + k] : (k % 4 == 0 ? 1.0 : 0.0);
        }
        srgb_lut.resize(256);
        for (int k = 0; k < 256; k++) srgb_lut[k] = std::pow((double)k / 255.0, PT_GAMMA);  // texture.rs:167: c.powf(GAMMA), c = byte / 255
        tri_uv.assign(total_tris * 6, 0.0);
        std::vector<uint8_t> tri_has_uv(total_tris, 0);
        for (uint32_t m = 0; m < s->n_meshes; m++) {
            if (!(s->mesh_texcoords && s->mesh_has_texcoords && s->mesh_has_texcoords[m])) continue;
            uint64_t v0 = s->mesh_vert_off[m];
            for (uint64_t t = s->mesh_tri_off[m]; t < s->mesh_tri_off[m + 1]; t++) {
                for (int corner = 0; corner < 3; corner++) {
                    uint64_t vi = v0 + s->mesh_indices[3 * t + corner];
                    tri_uv[6 * t + 2 * corner] = s->mesh_texcoords[2 * vi]; tri_uv[6 * t + 2 * corner + 1] = s->mesh_texcoords[2 * vi + 1];
                }
                tri_has_uv[t] = 1;
            }
        }
        for (uint32_t t = 0; t < s->n_triangles; t++)
            if (s->tri_texcoords && s->tri_has_texcoords && s->tri_has_texcoords[t]) {
                for (int k = 0; k < 6; k++) tri_uv[6 * (mesh_tris + t) + k] = s->tri_texcoords[6 * (size_t)t + k];
                tri_has_uv[mesh_tris + t] = 1;
            }
        // material.rs:133 / :141: the reference panics when a mapped material meets a primitive without texture coordinates
        for (uint32_t i = 0; i < n; i++) {
            int32_t m = s->material[i];
            if (mat_maps[2 * m] < 0 && mat_maps[2 * m + 1] < 0) continue;
            int t = s->prim_type[i];
            bool ok = t == PT_PRIM_SPHERE || t == PT_PRIM_CUBE || t == PT_PRIM_PLANE;
            if (t == PT_PRIM_TRIANGLE) ok = tri_has_uv[mesh_tris + (size_t)s->prim_data[i]];
            if (t == PT_PRIM_MESH || t == PT_PRIM_KDMESH) ok = s->mesh_tri_off[s->prim_data[i] + 1] == s->mesh_tri_off[s->prim_data[i]] || tri_has_uv[s->mesh_tri_off[s->prim_data[i]]];
            if (!ok) return pt_fail(c, PT_ERR_SCENE, "Texture mapping is not supported for this primitive! (material.rs:133,141)");
        }
        if ((rc = pt_upload(c, c->mat_maps, mat_maps)) || (rc = pt_upload(c, c->uv_trans, uv_trans)) || (rc = pt_upload(c, c->tex, texinfo)) ||
            (rc = pt_upload(c, c->tex_rgb, tex_rgb)) || (rc = pt_upload(c, c->srgb_lut, srgb_lut)) || (rc = pt_upload(c, c->tri_uv, tri_uv)))
            return rc;
    }

    PtSceneView& v = c->view;
    memset(&v, 0, sizeof v);
    v.n_nodes = n; v.n_lights = s->n_lights;
    v.inv = (const double*)c->inv.p; v.fwd = (const double*)c->fwd.p; v.nrm = (const double*)c->nrm.p;
    v.info = (const uint32_t*)c->info.p; v.tri_v = (const double*)c->tri_v.p; v.tri_e = (const double*)c->tri_e.p; v.tri_leaf = (const double*)c->tri_leaf.p; v.tri_n = (const double*)c->tri_n.p;
    v.meshes = (const PtMeshInfo*)c->meshes.p; v.materials = (const double*)c->materials.p; v.lights = (const double*)c->lights.p;
    for (int k = 0; k < 3; k++) v.ambient[k] = s->ambient[k];
    v.bvh = (const PtBvhNode*)c->bvh.p; v.bvh4 = (const PtBvh4Node*)c->bvh4.p; v.bvh_items = (const uint32_t*)c->bvh_items.p;
    v.tlas_root = tlas.child; v.tlas_direct = tlas_direct ? 1u : 0u;
    // the octant-sorted slab test inside mesh instances (pt_trace_packet_mesh; round 4, c32: the 1.25 M-triangle scenes +6.0 % / +3.1 %, macho-cows and the
    // mirror scene +0.6 %; PORTRAYER_MESH_OCT=0 walks every triangle tree with the per-lane form again)
    v.mesh_oct = 1u;
    if (const char* e = getenv("PORTRAYER_MESH_OCT")) v.mesh_oct = atoi(e) > 0 ? 1u : 0u;
    if ((rc = pt_upload_kd(c, kda, traverse == PT_TRAVERSE_KD))) return rc;
    v.mkd = mkd.empty() ? nullptr : (const PtKdNode*)c->mkd.p; v.mkd_items = (const uint32_t*)c->mkd_items.p;  // (null without KDMesh trees: the k-d walk then keeps no LDS rows for lane stacks)
    v.mkd_box = mkd_box.empty() || getenv("PORTRAYER_KD_NO_CULL") ? nullptr : (const float*)c->mkd_box.p;
    v.mkd_item_box = v.mkd_box ? (const float*)c->mkd_item_box.p : nullptr;
    v.mode = traverse == PT_TRAVERSE_KD ? (s->n_meshes == 0 ? PT_MODE_KD_NOMESH : (any_kdmesh ? PT_MODE_KD : PT_MODE_KD_MESH)) : (s->n_meshes == 0 ? PT_MODE_FLAT_NOMESH : (any_kdmesh ? PT_MODE_FLAT_KDMESH : PT_MODE_FLAT));
    if (traverse == PT_TRAVERSE_HIER) {  // the general walker (meshes and KDMesh trees compiled in), or its mesh-free instantiation
        v.mode = s->n_meshes == 0 ? PT_MODE_HIER_NOMESH : (any_kdmesh ? PT_MODE_HIER : PT_MODE_HIER_MESH);
        v.g_inv = (const double*)c->g_inv.p; v.g_fwd = (const double*)c->g_fwd.p; v.g_nrm = (const double*)c->g_nrm.p;
        v.chain_off = (const uint32_t*)c->chain_off.p; v.chain = (const uint32_t*)c->chain.p; v.dfs_rank = (const uint32_t*)c->dfs_rank.p;
        v.hier_rec = (const uint32_t*)c->hier_rec.p; v.own_inv = (const double*)c->own_inv.p;
    }
    {   // what pt_scene_update needs later (pt_context::Resident)
        pt_context::Resident& r = c->res;
        r.traverse = traverse; r.n_nodes = n; r.n_graph = traverse == PT_TRAVERSE_HIER && n ? s->n_graph_nodes : 0u; r.n_lights = s->n_lights;
        r.mesh_tris = mesh_tris; r.tlas_first = tlas_first; r.tlas_cap = tlas_cap; r.tlas_items = tlas_items; r.tree_nodes = tree_nodes;
        r.tlas_leaf = tlas_leaf; r.collapse_mode = collapse_mode;
        r.last_builder = 0; r.last_rounds = 0;
        auto wide = [&](int depth2) { return collapse_mode ? 3 * depth2 : 3 * ((depth2 + 1) / 2); };
        r.below = std::max(wide(max_blas_depth), 3 * (max_kdm_depth + 1));  // deepest walk under a scene leaf: a mesh tree or a KDMesh tree
        std::vector<double> mb(6 * mesh_box.size());
        for (size_t m = 0; m < mesh_box.size(); m++) for (int k = 0; k < 3; k++) { mb[6 * m + k] = mesh_box[m].lo[k]; mb[6 * m + 3 + k] = mesh_box[m].hi[k]; }
        if ((rc = pt_upload(c, c->mesh_box_dev, mb))) return rc;
        r.info = std::move(info); r.mesh_box = std::move(mesh_box); r.tri_box = std::move(tri_box);
        r.place = std::move(place); r.meshes = meshes; r.blas_leaf = blas_leaf; r.max_kdm_depth = max_kdm_depth; r.any_normals = any_normals;
        r.indices.assign(s->mesh_indices, s->mesh_indices + (mesh_tris ? 3 * mesh_tris : 0)); r.indices_resident = false;
        r.chain_off = std::move(chain_off); r.chain = std::move(chain);
    }
    const int cap_rc = pt_set_stack_cap(c, tlas.depth, kda.kd_depth);
    if (textured) {
        v.mat_maps = (const int32_t*)c->mat_maps.p; v.uv_trans = (const double*)c->uv_trans.p; v.tex = (const PtTexInfo*)c->tex.p;
        v.tex_rgb = (const uint8_t*)c->tex_rgb.p; v.srgb_lut = (const double*)c->srgb_lut.p; v.tri_uv = (const double*)c->tri_uv.p;
        std::vector<PtTexView> tv(1);
        tv[0].tex = v.tex; tv[0].tex_rgb = v.tex_rgb; tv[0].uv_trans = v.uv_trans; tv[0].tri_v = v.tri_v; tv[0].tri_uv = v.tri_uv;
        tv[0].mat_maps = v.mat_maps;
        if ((rc = pt_upload(c, c->texview, tv))) return rc;
        v.texview = (const PtTexView*)c->texview.p;
    }
    lap("upload the rest");
    if (cap_rc) return cap_rc;
    c->have_scene = true;
    return PT_OK;
}

// ------------------------------------------------------------------------------------------------
// Scene update: the resident scene with new node matrices, lights and ambient light. Everything under a flattened node lives in model space
// (triangle records, mesh trees, KDMesh trees, textures) and stays where it is; what depends on the matrices is recomputed by the functions
// pt_scene_upload uses (above), and the scene-level tree is rebuilt in the place the upload reserved for it - on the host (pt_bvh_build: the
// upload's tree) or on the device (pt_device_build_scene_tree), by the rule mesh trees follow: PORTRAYER_BUILD = host | device | auto,
// auto takes the device from PORTRAYER_BUILD_MIN nodes on (default 65536), device from 16 on; PORTRAYER_TLAS_LEAF != 1: always the host.
// ------------------------------------------------------------------------------------------------
// What an update computes on the host before its first write (pt_update_prepare) and then writes (pt_update_commit). pt_scene_deform runs the same two
// steps around its own writes, with the deformed meshes' new boxes.
struct PtUpdatePlan {
    std::vector<double> inv, fwd, nrm;
    PtGraphArrays graph;
    std::vector<PtBuildBox> node_box;
    double root_lo[3], root_hi[3];
    PtKdArrays kda;
    bool direct = false, on_device = false;
    std::vector<PtBvhNode> tl_nodes;
    std::vector<uint32_t> tl_items;
    PtBvhRef tlas;
};

// the copies and kernels of an update or a deform are not ordered against the context's non-blocking streams
static int pt_refuse_in_flight(pt_context* c) {
    bool in_flight = false;
    for (const PtPass* v : c->passes) in_flight = in_flight || v->pending;
    for (const auto& sl : c->slot) in_flight = in_flight || sl.pending;
    if (in_flight) return pt_fail(c, PT_ERR_ARGUMENT, "a render is in flight: pt_render_finish / pt_aov_finish / pt_rays_finish / pt_radiance_finish first");
    return PT_OK;
}

// Every check of pt_scene_update and everything its host side computes. `mesh_box`: the meshes' padded model boxes the moved scene has (the resident ones,
// or a deform's). Writes nothing to the device; PT_ERR_SCENE leaves the context without a scene, as after a refused upload.
// On the host-build path it does set view.stack_cap (pt_set_stack_cap) from the mesh depths as they are BEFORE the call: for a deform with rebuild = 1
// that is half a check - a mesh tree the rebuild makes deeper is only seen by pt_update_commit, which computes the cap again after the writes and then
// ends with PT_ERR_SCENE and no scene, as the header says.
static int pt_update_prepare(pt_context* c, const pt_scene_motion* mo, const pt_kdtree* kd, const std::vector<PtBuildBox>& mesh_box, PtUpdatePlan& p) {
    if (!c || !mo) return PT_ERR_ARGUMENT;
    if (!c->have_scene) return pt_fail(c, PT_ERR_NO_SCENE, "no scene uploaded");
    pt_context::Resident& res = c->res;
    const uint32_t n = res.n_nodes;
    if (mo->n_nodes != n) return pt_fail(c, PT_ERR_ARGUMENT, "n_nodes differs from the uploaded scene's");
    if (n && (!mo->trans || !mo->invtrans || !mo->normal_trans)) return pt_fail(c, PT_ERR_ARGUMENT, "null node array");
    if (mo->n_graph_nodes != res.n_graph) return pt_fail(c, PT_ERR_ARGUMENT, "n_graph_nodes differs from the uploaded scene's (0 unless it was uploaded with PT_TRAVERSE_HIER)");
    if (res.n_graph && (!mo->graph_trans || !mo->graph_invtrans || !mo->graph_normal_trans))
        return pt_fail(c, PT_ERR_ARGUMENT, "PT_TRAVERSE_HIER needs the scene graph's matrices (graph_*)");
    if (mo->lights && mo->n_lights != res.n_lights) return pt_fail(c, PT_ERR_ARGUMENT, "n_lights differs from the uploaded scene's");
    if (res.traverse == PT_TRAVERSE_KD && !kd) return pt_fail(c, PT_ERR_ARGUMENT, "PT_TRAVERSE_KD needs the host-built k-d tree");
    if (res.traverse != PT_TRAVERSE_KD && kd) return pt_fail(c, PT_ERR_ARGUMENT, "a k-d tree for a scene that was not uploaded with PT_TRAVERSE_KD");
    if (int rc = pt_refuse_in_flight(c)) return rc;

    // ---- everything the host computes, before the first write
    pt_pack_node_matrices(n, mo->trans, mo->invtrans, mo->normal_trans, p.inv, p.fwd, p.nrm);
    if (res.n_graph) pt_pack_graph(n, res.n_graph, mo->graph_trans, mo->graph_invtrans, mo->graph_normal_trans, res.chain_off, res.chain, p.graph);
    pt_node_world_boxes(n, mo->trans, res.info.data(), mesh_box, res.tri_box, res.mesh_tris, p.node_box, p.root_lo, p.root_hi);
    int rc;
    if (res.traverse == PT_TRAVERSE_KD && (rc = pt_pack_kd(c, kd, n, p.node_box, p.kda))) {
        if (rc == PT_ERR_SCENE) c->have_scene = false;  // as after a refused upload
        return rc;
    }
    int build_mode = 2;
    size_t device_build_min = 65536;
    if (const char* e = getenv("PORTRAYER_BUILD")) build_mode = !strcmp(e, "host") ? 0 : (!strcmp(e, "device") ? 1 : 2);
    if (const char* e = getenv("PORTRAYER_BUILD_MIN")) device_build_min = (size_t)std::max(16, atoi(e));
    p.direct = res.tlas_leaf == 1 && n < (1u << 28);
    p.on_device = p.direct && ((build_mode == 1 && n >= 16) || (build_mode == 2 && n >= device_build_min));
    p.tlas.child = PT_REF_EMPTY; p.tlas.depth = 0;
    if (!p.on_device) {
        p.tlas = pt_build_scene_tree(p.node_box, res.tlas_leaf, p.direct, res.tlas_first, res.tlas_items, p.tl_nodes, p.tl_items);
        if (p.tl_nodes.size() > res.tlas_cap || p.tl_items.size() > (p.direct ? 0u : n)) return pt_fail(c, PT_ERR_DEVICE, "scene tree larger than its place");  // (a tree over n leaves has at most n - 1 nodes)
        if ((rc = pt_set_stack_cap(c, p.tlas.depth, p.kda.kd_depth))) { c->have_scene = false; return rc; }
    }
    return PT_OK;
}

// ---- writes
static int pt_update_commit(pt_context* c, const pt_scene_motion* mo, PtUpdatePlan& p) {
    pt_context::Resident& res = c->res;
    const uint32_t n = res.n_nodes;
    int rc;
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipDeviceSynchronize());  // passes whose _finish has been called may still have copies queued
    c->have_scene = false;              // until every write below has been made
    if ((rc = pt_upload(c, c->inv, p.inv)) || (rc = pt_upload(c, c->fwd, p.fwd)) || (rc = pt_upload(c, c->nrm, p.nrm))) return rc;
    if (res.n_graph && ((rc = pt_upload(c, c->g_inv, p.graph.g_inv)) || (rc = pt_upload(c, c->g_fwd, p.graph.g_fwd)) || (rc = pt_upload(c, c->g_nrm, p.graph.g_nrm)) ||
                        (rc = pt_upload(c, c->hier_rec, p.graph.hier_rec)) || (rc = pt_upload(c, c->own_inv, p.graph.own_inv))))
        return rc;
    if (res.traverse == PT_TRAVERSE_KD && (rc = pt_upload_kd(c, p.kda, true))) return rc;
    for (int k = 0; k < 3; k++) { c->root_lo[k] = p.root_lo[k]; c->root_hi[k] = p.root_hi[k]; }
    PtSceneView& v = c->view;
    if (mo->lights) {
        std::vector<double> lights(mo->lights, mo->lights + 15 * (size_t)mo->n_lights);
        if ((rc = pt_upload(c, c->lights, lights))) return rc;
        pt_set_light_flags(c, lights.data(), mo->n_lights);
    }
    if (mo->ambient) for (int k = 0; k < 3; k++) v.ambient[k] = mo->ambient[k];
    PtBvhRef tlas = p.tlas;
    if (p.on_device) {
        PtDeviceBuildResult built;
        PT_HIP(c, pt_device_build_scene_tree(n, (const double*)c->fwd.p, (const uint32_t*)c->info.p, (const double*)c->mesh_box_dev.p, (const double*)c->tri_v.p,
                                             p.root_lo, p.root_hi, (PtBvhNode*)c->bvh.p, (uint32_t)res.tlas_first, nullptr, &built));
        tlas.child = built.root; tlas.depth = built.depth;
        if (getenv("PORTRAYER_VERBOSE")) fprintf(stderr, "[pt_scene_update] device scene tree: %u nodes, %.2f ms, %d clustering rounds, depth %d\n", n, built.ms, built.rounds, built.depth);
        res.last_builder = 2; res.last_rounds = built.rounds;
    } else {
        res.last_builder = 1; res.last_rounds = 0;
        if (!p.tl_nodes.empty()) PT_HIP(c, hipMemcpy((PtBvhNode*)c->bvh.p + res.tlas_first, p.tl_nodes.data(), p.tl_nodes.size() * sizeof(PtBvhNode), hipMemcpyHostToDevice));
        if (!p.tl_items.empty()) PT_HIP(c, hipMemcpy((uint32_t*)c->bvh_items.p + res.tlas_items, p.tl_items.data(), p.tl_items.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    // the stack of the trees as they are now: the scene-level tree just built and (pt_scene_deform) mesh trees a rebuild may have made deeper
    if ((rc = pt_set_stack_cap(c, tlas.depth, p.kda.kd_depth))) return rc;  // (have_scene stays false)
    if (res.tlas_cap) {  // the four-child form of the new tree alone, opened as the upload opened it
        const uint32_t first = (uint32_t)res.tlas_first, end = (uint32_t)(res.tlas_first + res.tlas_cap);
        hipLaunchKernelGGL(pt_collapse4_kernel, dim3((unsigned)((res.tlas_cap + 255) / 256)), dim3(256), 0, nullptr, (const PtBvhNode*)c->bvh.p, (PtBvh4Node*)c->bvh4.p,
                           (uint32_t)res.tree_nodes, res.collapse_mode, first, end, first, end);
        PT_HIP(c, hipGetLastError());
    }
    PT_HIP(c, hipDeviceSynchronize());
    v.tlas_root = tlas.child;
    c->have_scene = true;
    return PT_OK;
}

extern "C" int pt_scene_update(pt_context* c, const pt_scene_motion* mo, const pt_kdtree* kd) {
    if (!c || !mo) return PT_ERR_ARGUMENT;
    PtUpdatePlan plan;
    int rc = pt_update_prepare(c, mo, kd, c->res.mesh_box, plan);
    if (rc) return rc;
    return pt_update_commit(c, mo, plan);
}

// ------------------------------------------------------------------------------------------------
// Scene deform: new vertices for resident meshes under the topology they were uploaded with, then the update above. Per mesh the host
// computes the box (the upload's function) and copies the vertices; the device expands the triangle records through the resident indices
// (pt_device_expand_mesh), refits the mesh's tree in place or rebuilds it there (pt_device_refit_mesh_tree / pt_device_build_mesh_tree) and re-derives
// the four-child form and the leaf-order records for the mesh's node and item ranges alone. With the vertices already in device memory
// (pt_scene_deform_device) the box is a reduction on the device (pt_device_vertex_box) and the expand kernel reads the caller's buffer in place.
// ------------------------------------------------------------------------------------------------
// One mesh of a deform, wherever its vertices are: pt_mesh_deform's fields with host pointers, pt_mesh_deform_device's with device pointers.
struct PtDeformItem {
    uint32_t mesh;
    const double *positions, *normals, *bounds_invtrans;
    int32_t rebuild;
};

// What keeps a caller's mistake from becoming a GPU fault: `p` must be 8-byte aligned device memory of the context's device whose allocation reaches `bytes`
// beyond it. The context's device is current.
static int pt_check_device_pointer(pt_context* c, const void* p, uint64_t bytes, const std::string& what) {
    if ((uintptr_t)p & 7u) return pt_fail(c, PT_ERR_ARGUMENT, what + " is not 8-byte aligned");
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();  // (pageable host memory: the query itself fails, and leaves its error behind)
        return pt_fail(c, PT_ERR_ARGUMENT, what + " is not device memory (hipPointerGetAttributes does not know the pointer)");
    }
    if (at.type != hipMemoryTypeDevice || at.isManaged)
        return pt_fail(c, PT_ERR_ARGUMENT, what + " is not device memory (host, pinned or managed memory: copy it to the device, or use pt_scene_deform)");
    if (at.device != c->device)
        return pt_fail(c, PT_ERR_ARGUMENT, what + " is memory of device " + std::to_string(at.device) + ", the context is on device " + std::to_string(c->device));
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess || !base) {
        (void)hipGetLastError();
        return pt_fail(c, PT_ERR_ARGUMENT, what + ": hipMemGetAddressRange does not know the pointer's allocation");
    }
    const uint64_t off = (uint64_t)((const char*)p - (const char*)base);
    if ((const char*)p < (const char*)base || off > size || bytes > size - off)
        return pt_fail(c, PT_ERR_ARGUMENT, what + ": the allocation ends " + std::to_string(size - std::min<uint64_t>(off, size)) + " bytes after the pointer, " + std::to_string(bytes) + " are needed (n_vertices x 24)");
    return PT_OK;
}

// The box and the count of non-finite coordinates of n x 3 f64 in device memory (pt_device_vertex_box): the pointer has passed pt_check_device_pointer, the
// context's device is current and synchronised. One copy brings the result back.
static int pt_vertex_box_on_device(pt_context* c, uint64_t n, const double* d_pos, PtBuildBox* box, uint64_t* non_finite) {
    int rc = pt_reserve(c, c->vbox, (size_t)pt_vertex_box_partials(c->n_cu) * sizeof(PtVboxPartial));
    if (rc) return rc;
    PT_HIP(c, pt_device_vertex_box(d_pos, n, c->n_cu, (PtVboxPartial*)c->vbox.p, nullptr));
    PtVboxPartial got;
    PT_HIP(c, hipMemcpy(&got, c->vbox.p, sizeof got, hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; k++) { box->lo[k] = got.v[k]; box->hi[k] = got.v[3 + k]; }
    *non_finite = got.non_finite;
    return PT_OK;
}

extern "C" int pt_vertex_bounds_device(pt_context* c, uint64_t n_vertices, const double* d_positions, double out[6], uint64_t* non_finite) {
    if (!c) return PT_ERR_ARGUMENT;
    if (!out || !non_finite) return pt_fail(c, PT_ERR_ARGUMENT, "out and non_finite are required");
    if (n_vertices > 0xFFFFFFFFull) return pt_fail(c, PT_ERR_ARGUMENT, "n_vertices must be below 2^32");
    PtBuildBox box = pt_bvh_detail::empty_box();
    *non_finite = 0;
    if (n_vertices) {
        if (!d_positions) return pt_fail(c, PT_ERR_ARGUMENT, "d_positions is required");
        PT_HIP(c, hipSetDevice(c->device));
        int rc = pt_check_device_pointer(c, d_positions, n_vertices * 24, "d_positions");
        if (rc) return rc;
        PT_HIP(c, hipDeviceSynchronize());  // behind whatever stream produced the vertices
        if ((rc = pt_vertex_box_on_device(c, n_vertices, d_positions, &box, non_finite))) return rc;
    }
    for (int k = 0; k < 3; k++) { out[k] = box.lo[k]; out[3 + k] = box.hi[k]; }
    return PT_OK;
}

// pt_scene_deform and pt_scene_deform_device: the two differ in where a mesh's box comes from (the host loop / the device reduction behind the pointer check)
// and in which pointer the expand kernel reads (the staging buffer the vertices are copied to / the caller's buffer in place).
static int pt_deform_meshes(pt_context* c, const std::vector<PtDeformItem>& items, bool on_device, const pt_scene_motion* mo, const pt_kdtree* kd) {
    if (!c->have_scene) return pt_fail(c, PT_ERR_NO_SCENE, "no scene uploaded");
    pt_context::Resident& res = c->res;
    const uint32_t n_deforms = (uint32_t)items.size();
    struct NewBox { PtBuildBox vertex, padded; double ext; };
    std::vector<NewBox> nb(n_deforms);
    std::vector<PtBuildBox> mesh_box = res.mesh_box;
    {
        std::vector<uint8_t> named(res.place.size(), 0);
        bool synchronised = false;
        for (uint32_t d = 0; d < n_deforms; d++) {
            const PtDeformItem& df = items[d];
            const std::string at = "deform " + std::to_string(d) + ": ";
            if (!df.positions || !df.bounds_invtrans) return pt_fail(c, PT_ERR_ARGUMENT, at + "positions and bounds_invtrans are required");
            if (df.mesh >= res.place.size()) return pt_fail(c, PT_ERR_ARGUMENT, at + "mesh index out of range");
            if (named[df.mesh]) return pt_fail(c, PT_ERR_ARGUMENT, at + "the mesh is named twice");
            named[df.mesh] = 1;
            const pt_context::Resident::MeshPlace& pl = res.place[df.mesh];
            if (df.normals && !pl.has_normals) return pt_fail(c, PT_ERR_ARGUMENT, at + "normals for a mesh that was uploaded without normals");
            if (res.meshes[df.mesh].kd_root >= 0)
                return pt_fail(c, PT_ERR_ARGUMENT, at + "the mesh has a KDMesh tree, which the host builds from the positions: upload the scene again");
            if (df.rebuild != 0 && df.rebuild != 1) return pt_fail(c, PT_ERR_ARGUMENT, at + "rebuild must be 0 or 1");
            if (df.rebuild && !pl.device_built)
                return pt_fail(c, PT_ERR_ARGUMENT, at + "rebuild = 1 needs a tree the device built at upload (its place has the worst-case size); this one was built on the host");
            bool finite = true;
            if (on_device) {
                nb[d].vertex = pt_bvh_detail::empty_box();
                if (pl.n_verts) {  // (nothing is launched on an empty mesh, and nothing of it is read)
                    int rc = pt_refuse_in_flight(c);
                    if (rc) return rc;
                    PT_HIP(c, hipSetDevice(c->device));
                    if ((rc = pt_check_device_pointer(c, df.positions, (uint64_t)pl.n_verts * 24, at + "d_positions"))) return rc;
                    if (df.normals && (rc = pt_check_device_pointer(c, df.normals, (uint64_t)pl.n_verts * 24, at + "d_normals"))) return rc;
                    if (!synchronised) PT_HIP(c, hipDeviceSynchronize());  // behind whatever stream produced the vertices
                    synchronised = true;
                    uint64_t non_finite = 0;
                    if ((rc = pt_vertex_box_on_device(c, pl.n_verts, df.positions, &nb[d].vertex, &non_finite))) return rc;
                    finite = non_finite == 0;
                }
                nb[d].ext = pt_box_extent(nb[d].vertex);
            } else {
                nb[d].ext = pt_mesh_vertex_box(df.positions, pl.n_verts, &nb[d].vertex);
                for (uint64_t v = 0; v < 3 * (uint64_t)pl.n_verts; v++) finite = finite && std::isfinite(df.positions[v]);
            }
            nb[d].padded = nb[d].vertex;
            for (int k = 0; k < 3; k++) { nb[d].padded.lo[k] -= 1e-5 * nb[d].ext; nb[d].padded.hi[k] += 1e-5 * nb[d].ext; }
            for (int k = 0; k < 3; k++) finite = finite && nb[d].padded.lo[k] >= -PT_BOX_LIMIT && nb[d].padded.hi[k] <= PT_BOX_LIMIT;
            if (!finite) return pt_fail(c, PT_ERR_ARGUMENT, at + "a coordinate is not finite or the mesh's box reaches beyond +-1e18");
            mesh_box[df.mesh] = nb[d].padded;
        }
    }
    PtUpdatePlan plan;
    int rc = pt_update_prepare(c, mo, kd, mesh_box, plan);
    if (rc) return rc;
    if (n_deforms == 0) return pt_update_commit(c, mo, plan);

    // ---- writes
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipDeviceSynchronize());
    c->have_scene = false;  // until every write has been made (pt_update_commit sets it again)
    const bool verbose = getenv("PORTRAYER_VERBOSE") != nullptr;
    if (!res.indices_resident) {
        if ((rc = pt_upload(c, c->mesh_idx, res.indices))) return rc;
        res.indices_resident = true;
    }
    bool any_refit = false;
    size_t stage_bytes = 0;
    for (uint32_t d = 0; d < n_deforms; d++) {
        any_refit = any_refit || !items[d].rebuild;
        stage_bytes = std::max(stage_bytes, (size_t)res.place[items[d].mesh].n_verts * 24 * (items[d].normals ? 2 : 1));
    }
    if (!on_device && (rc = pt_reserve(c, c->deform_stage, stage_bytes))) return rc;  // (vertices in device memory are read where they are)
    if (any_refit && ((rc = pt_reserve(c, c->tree_parent, std::max<size_t>(res.tree_nodes, 1) * 4)) || (rc = pt_reserve(c, c->tree_arrive, std::max<size_t>(res.tree_nodes, 1) * 4)))) return rc;
    const bool write_normals = res.any_normals;  // (tri_n is empty unless a node shades smoothly: the upload then drops the normals it is given, and so does this)
    for (uint32_t d = 0; d < n_deforms; d++) {
        const PtDeformItem& df = items[d];
        pt_context::Resident::MeshPlace& pl = res.place[df.mesh];
        PtMeshInfo& mi = res.meshes[df.mesh];
        const size_t pos_bytes = (size_t)pl.n_verts * 24;
        const double *d_pos = df.positions, *d_nrm = df.normals && write_normals ? df.normals : nullptr;
        if (!on_device) {
            PT_HIP(c, hipMemcpy(c->deform_stage.p, df.positions, pos_bytes, hipMemcpyHostToDevice));
            if (df.normals) PT_HIP(c, hipMemcpy((char*)c->deform_stage.p + pos_bytes, df.normals, pos_bytes, hipMemcpyHostToDevice));
            d_pos = (const double*)c->deform_stage.p;
            if (d_nrm) d_nrm = (const double*)((const char*)c->deform_stage.p + pos_bytes);
        }
        PT_HIP(c, pt_device_expand_mesh((const uint32_t*)c->mesh_idx.p, mi.tri_first, mi.tri_count, d_pos, d_nrm, pl.n_verts, (double*)c->tri_v.p, (double*)c->tri_e.p,
                                        d_nrm ? (double*)c->tri_n.p : nullptr, nullptr));
        const double pad = 1e-7 * nb[d].ext;
        if (df.rebuild) {
            PtDeviceBuildResult built;
            PT_HIP(c, hipMemsetAsync((PtBvhNode*)c->bvh.p + pl.node_first, 0xFF, (size_t)pl.node_count * sizeof(PtBvhNode), nullptr));
            PT_HIP(c, pt_device_build_mesh_tree((const double*)c->tri_v.p, mi.tri_first, mi.tri_count, nb[d].vertex.lo, nb[d].vertex.hi, pad, res.blas_leaf, (PtBvhNode*)c->bvh.p,
                                                pl.node_first, (uint32_t*)c->bvh_items.p, pl.item_first, nullptr, &built));
            mi.blas_root = built.root; pl.depth = built.depth; pl.parents_valid = false;
            if (verbose) fprintf(stderr, "[pt_scene_deform] mesh %u rebuilt: %u triangles, %.2f ms, %d clustering rounds, depth %d\n", df.mesh, mi.tri_count, built.ms, built.rounds, built.depth);
        } else if (pl.node_count) {
            if (!pl.parents_valid) {
                PT_HIP(c, pt_device_tree_parents((const PtBvhNode*)c->bvh.p, pl.node_first, pl.node_count, (uint32_t*)c->tree_parent.p, nullptr));
                pl.parents_valid = true;
            }
            PT_HIP(c, pt_device_refit_mesh_tree((PtBvhNode*)c->bvh.p, pl.node_first, pl.node_count, (const uint32_t*)c->bvh_items.p, pl.item_first, pl.item_count,
                                                (const double*)c->tri_v.p, mi.tri_first, mi.tri_count, pad, (const uint32_t*)c->tree_parent.p, (uint32_t*)c->tree_arrive.p, nullptr));
        }
        // what the walks read, for the mesh's node and item ranges alone
        if (pl.node_count) {
            const uint32_t first = pl.node_first, end = pl.node_first + pl.node_count;
            hipLaunchKernelGGL(pt_collapse4_kernel, dim3((pl.node_count + 255) / 256), dim3(256), 0, nullptr, (const PtBvhNode*)c->bvh.p, (PtBvh4Node*)c->bvh4.p,
                               (uint32_t)res.tree_nodes, res.collapse_mode, (uint32_t)res.tlas_first, (uint32_t)(res.tlas_first + res.tlas_cap), first, end);
            PT_HIP(c, hipGetLastError());
        }
        if (pl.item_count) {
            hipLaunchKernelGGL(pt_tri_leaf_kernel, dim3((pl.item_count + 255) / 256), dim3(256), 0, nullptr, (const uint32_t*)c->bvh_items.p + pl.item_first, pl.item_count,
                               (const double*)c->tri_e.p, (uint32_t)(res.mesh_tris + res.tri_box.size()), (double*)c->tri_leaf.p + 10 * (size_t)pl.item_first);
            PT_HIP(c, hipGetLastError());
        }
        for (int r = 0; r < 12; r++) mi.bbox_inv[r] = df.bounds_invtrans[r];
        res.mesh_box[df.mesh] = nb[d].padded;
        PT_HIP(c, hipStreamSynchronize(nullptr));  // the staging buffer is the next mesh's
    }
    {   // the records the walks and the scene-level build read: PtMeshInfo (bbox_inv, blas_root), the padded boxes; the stack under a scene leaf
        if ((rc = pt_upload(c, c->meshes, res.meshes))) return rc;
        std::vector<double> mb(6 * res.mesh_box.size());
        for (size_t m = 0; m < res.mesh_box.size(); m++) for (int k = 0; k < 3; k++) { mb[6 * m + k] = res.mesh_box[m].lo[k]; mb[6 * m + 3 + k] = res.mesh_box[m].hi[k]; }
        if ((rc = pt_upload(c, c->mesh_box_dev, mb))) return rc;
        int max_blas_depth = 0;
        for (const auto& pl : res.place) max_blas_depth = std::max(max_blas_depth, pl.depth);
        auto wide = [&](int depth2) { return res.collapse_mode ? 3 * depth2 : 3 * ((depth2 + 1) / 2); };
        res.below = std::max(wide(max_blas_depth), 3 * (res.max_kdm_depth + 1));
    }
    return pt_update_commit(c, mo, plan);
}

extern "C" int pt_scene_deform(pt_context* c, uint32_t n_deforms, const pt_mesh_deform* deforms, const pt_scene_motion* mo, const pt_kdtree* kd) {
    if (!c || !mo || (n_deforms && !deforms)) return PT_ERR_ARGUMENT;
    std::vector<PtDeformItem> items(n_deforms);
    for (uint32_t d = 0; d < n_deforms; d++) items[d] = PtDeformItem{deforms[d].mesh, deforms[d].positions, deforms[d].normals, deforms[d].bounds_invtrans, deforms[d].rebuild};
    return pt_deform_meshes(c, items, false, mo, kd);
}

extern "C" int pt_scene_deform_device(pt_context* c, uint32_t n_deforms, const pt_mesh_deform_device* deforms, const pt_scene_motion* mo, const pt_kdtree* kd) {
    if (!c || !mo || (n_deforms && !deforms)) return PT_ERR_ARGUMENT;
    std::vector<PtDeformItem> items(n_deforms);
    for (uint32_t d = 0; d < n_deforms; d++) items[d] = PtDeformItem{deforms[d].mesh, deforms[d].d_positions, deforms[d].d_normals, deforms[d].bounds_invtrans, deforms[d].rebuild};
    return pt_deform_meshes(c, items, true, mo, kd);
}

extern "C" int pt_scene_mesh_rebuildable(const pt_context* c, uint32_t mesh) {
    if (!c) return PT_ERR_ARGUMENT;
    if (!c->have_scene) return PT_ERR_NO_SCENE;
    if (mesh >= c->res.place.size()) return PT_ERR_ARGUMENT;
    return c->res.place[mesh].device_built ? 1 : 0;
}

// tests: the bytes of device memory the context's scene buffers hold (an update must not make it grow)
extern "C" uint64_t pt_test_scene_bytes(const pt_context* c) {
    if (!c) return 0;
    const PtBuf* bufs[] = {&c->inv, &c->fwd, &c->nrm, &c->info, &c->tri_v, &c->tri_e, &c->tri_leaf, &c->tri_n, &c->meshes, &c->materials, &c->lights, &c->bvh, &c->bvh4,
                           &c->bvh_items, &c->kd, &c->kd_items, &c->mat_maps, &c->uv_trans, &c->tex, &c->tex_rgb, &c->srgb_lut, &c->tri_uv, &c->texview, &c->mkd, &c->mkd_items,
                           &c->node_box, &c->kd_box, &c->mkd_box, &c->mkd_item_box, &c->kd_ref, &c->g_inv, &c->g_fwd, &c->g_nrm, &c->chain_off, &c->chain, &c->dfs_rank,
                           &c->hier_rec, &c->own_inv, &c->mesh_box_dev, &c->mesh_idx, &c->tree_parent, &c->tree_arrive, &c->deform_stage};
    uint64_t total = 0;
    for (const PtBuf* b : bufs) total += b->bytes;
    return total;
}

extern "C" int pt_test_vertex_box_shape(const pt_context* c, uint64_t out[2]) {
    if (!c || !out) return PT_ERR_ARGUMENT;
    out[0] = PT_VBOX_BLOCK; out[1] = pt_vertex_box_partials(c->n_cu);
    return PT_OK;
}

// tests: out[0] = stack_cap, out[1] = who built the scene-level tree last (0 the upload, 1 an update on the host, 2 an update on the device),
// out[2] = the device build's clustering rounds, out[3] = bytes of the tree buffers (bvh, bvh4, bvh_items)
extern "C" int pt_test_scene_info(const pt_context* c, uint64_t out[4]) {
    if (!c || !out) return PT_ERR_ARGUMENT;
    if (!c->have_scene) return PT_ERR_NO_SCENE;
    out[0] = (uint64_t)c->view.stack_cap; out[1] = (uint64_t)c->res.last_builder; out[2] = (uint64_t)c->res.last_rounds;
    out[3] = c->bvh.bytes + c->bvh4.bytes + c->bvh_items.bytes;
    return PT_OK;
}

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
    if (c->pl_slot < 0 || c->pl_slots == 0) return PT_OK;
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipDeviceSynchronize());
    std::vector<uint32_t> rec((size_t)c->pl_slots * PT_PL_WORDS);
    const pt_context::Slot& sl = c->slot[c->pl_slot];
    if (sl.eye_tab.bytes < c->pl_off + rec.size() * 4) return pt_fail(c, PT_ERR_ARGUMENT, "the slot's buffer no longer holds that launch's lists");
    PT_HIP(c, hipMemcpy(rec.data(), (const char*)sl.eye_tab.p + c->pl_off, rec.size() * 4, hipMemcpyDeviceToHost));
    out[0] = c->pl_slots;
    for (uint32_t i = 0; i < c->pl_slots; i++) {
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
extern "C" int pt_test_pixel_beam(uint64_t n, const double* cameras, const uint32_t* pixels, const double* jitters, const float* box_lo, const float* box_hi,
                                  int32_t* accept, float* bound, int32_t* walk, double* rays) {
    if (!cameras || !pixels || !jitters || !box_lo || !box_hi || !accept || !bound || !walk) return PT_ERR_ARGUMENT;
    for (uint64_t i = 0; i < n; i++) {
        PtCamera cam;
        const double* cp = cameras + 19 * i;
        for (int k = 0; k < 3; k++) cam.eye[k] = cp[k];
        for (int k = 0; k < 12; k++) cam.view_to_world[k] = cp[3 + k];
        cam.fov_factor = cp[15]; cam.aspect = cp[16]; cam.width = cp[17]; cam.height = cp[18];
        const uint32_t x = pixels[2 * i], y = pixels[2 * i + 1];
        const float* lo = box_lo + 3 * i;
        const float* hi = box_hi + 3 * i;
        const PtBeam beam = pt_beam_setup(cam, (double)x, (double)y);
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

// How a launch's traversal stacks are split between LDS and HBM - one place for the render kernels and every pass beside them, whose
// kernels lay their LDS out with the same code (pt_trace_wave: pt_wave_rows, pt_kd_layout).
// pt_stack_lds_cap: entries per lane kept in LDS = what `block_budget` bytes of LDS per block leave beside `frame_bytes` of other per-block data (1 KB a row), at most the
// scene's whole stack. The k-d walk keeps no saved bounds in HBM (round 5): its wavefront rows must hold the stack and, where the stack's slack is too small for it, the two
// rows of the path table (pt_kd_layout, PtKdSav) - also under PORTRAYER_LDS_STACK=1 (experiments / tests of the overflow path), which then only shrinks the LANES' stacks.
static bool pt_kd_semantics(int mode) { return mode == PT_MODE_KD || mode == PT_MODE_KD_NOMESH || mode == PT_MODE_KD_MESH; }
static int pt_stack_lds_cap(const PtSceneView& sc, size_t block_budget, size_t frame_bytes) {
    int lds_cap = block_budget > frame_bytes ? (int)((block_budget - frame_bytes) / (PT_BLOCK * 4)) : 0;
    lds_cap = std::max(lds_cap, 2);
    if (const char* e = getenv("PORTRAYER_LDS_STACK")) lds_cap = std::max(1, atoi(e));
    int cap = std::min(lds_cap, sc.stack_cap);
    if (pt_kd_semantics(sc.mode)) cap = std::max(cap, (sc.stack_cap + 63) / 64 + 2);
    return cap;
}
// pt_stack_column: entries of a lane's HBM stack column (PtStackSpill::gbase). + wave_rows: the wavefront's own stack takes LDS rows from the lanes' stacks (pt_wave_rows,
// pt_render_simple.h): eight, or what a deep tree needs; and at least everything a lane's own stack can reach (pt_trace_wave gives the lanes fewer LDS rows in the k-d semantics).
static size_t pt_stack_column(const PtSceneView& sc, int stack_lds_cap) {
    const int wave_rows = std::min(std::max(8, (sc.stack_cap + 63) / 64), std::max(stack_lds_cap, 8));  // (pt_wave_rows: at most this many)
    const int stack_spill_entries = std::max(sc.stack_cap - stack_lds_cap + wave_rows, 0);
    return (size_t)std::max(stack_spill_entries, sc.stack_cap);
}

// What a pass's sizing dispatch reads of the host-side fields. The passes that only walk (primary visibility, ray queries): the LDS stack area is sized like a
// render's for the waves per SIMD the mode's instantiation is compiled for, with no hit frame beside the stacks.
static void pt_walk_sizing(PtRenderArgs& r, int waves) {
    r.stack_lds_cap = pt_stack_lds_cap(r.scene, waves == 3 ? 52 * 1024 : 39 * 1024, 0);  // 3 x 52 KB or 4 x 39 KB of the CU's 160 KB
    r.grid_share = 1;
}
// The interpreter passes (radiance, the film's): LDS per block as a render's interpreter kernel has it - three blocks per CU, the stack area beside the hit
// frame and, in scenes whose hits spawn rays, the youngest parked frame of every lane. Returns which <TEX, PARK> instantiation runs.
struct PtInterp { bool tex, park; };
static PtInterp pt_interp_sizing(const pt_context* c, PtRenderArgs& r) {
    PtInterp k;
    k.tex = r.scene.mat_maps != nullptr;
    k.park = c->spawns;
    if (const char* e = getenv("PORTRAYER_PARK")) k.park = k.park && atoi(e) > 0;  // 0: every parked frame in HBM (tests, measurements), as for a render
    r.park_slots = k.park ? 1 : 0;
    const size_t frame_bytes = (size_t)(PT_LDS_FRAME_F64 + r.park_slots * PT_PARK_F64) * PT_BLOCK * 8;
    r.stack_lds_cap = pt_stack_lds_cap(r.scene, 52 * 1024, frame_bytes);  // 3 x 52 KB of the CU's 160 KB (pt_radiance_waves, pt_film_waves)
    r.grid_share = 1;
    return k;
}

static int pt_render_common(pt_context* c, PtRenderArgs& a, bool stats, hipStream_t stream, int slot_index = -1) {
    // LDS per block = traversal stack (as much of it as leaves room for three blocks per CU) + the shaded hit's frame (+ a parked one);
    // deeper stack entries live in HBM (PtStackSpill).
    if (getenv("PORTRAYER_NO_TEX")) a.scene.mat_maps = nullptr;  // experiment: the untextured kernel on a textured scene (wrong picture, timing only)
    const bool tex = a.scene.mat_maps != nullptr;
    // parked recursion frames kept in LDS (pt_shade.h): only scenes that park frames at all have any
    a.park_slots = 1;
    if (const char* e = getenv("PORTRAYER_PARK")) a.park_slots = atoi(e) > 0 ? 1 : 0;  // 0: every parked frame in HBM (tests, measurements)
    if (!c->spawns) a.park_slots = 0;
    // Scenes whose hits spawn rays need the interpreter kernel (3 waves per SIMD); the others run the straight-line kernel at 3 or
    // 4 waves per SIMD.
    const bool kd_sem = pt_kd_semantics(a.scene.mode);
    a.four_waves = (!c->spawns && (c->four_waves || (c->four_waves_untextured && !tex) || c->four_waves_hier)) ? (c->five_waves ? PT_LINE_TOP_WAVES : ((c->five_waves_mesh && !tex) ? PT_MESH_TOP_WAVES : 4)) : 0;
    if (const char* e = getenv("PORTRAYER_WAVES")) {
        const int wv = atoi(e);
        a.four_waves = (!c->spawns && wv >= 4) ? ((wv >= 5 && (a.scene.mode == PT_MODE_FLAT_NOMESH || a.scene.mode == PT_MODE_HIER_NOMESH)) ? PT_LINE_TOP_WAVES : ((wv >= 5 && (a.scene.mode == PT_MODE_FLAT || a.scene.mode == PT_MODE_HIER_MESH)) ? PT_MESH_TOP_WAVES : 4)) : 0;
    }
    if (kd_sem) {
        // The k-d semantics: mesh-free scenes with many nodes take the 4-wave straight-line kernel too (big-scene 35.7 -> 30.7 ms: the per-lane
        // k-d walk waits on its own loads, a fourth wavefront per SIMD hides more of that than the 4 spilled registers cost); with mesh
        // instances the walk needs the registers (167 at 3 waves). PORTRAYER_KD_WAVES=3|4 overrides.
        // Round 4 (one walk per wavefront, pt_trace_packet_kd): mesh-free scenes with many nodes at 5 waves (big-scene 29.2 -> 28.1 ms, c10), scenes with plain
        // Mesh instances (PT_MODE_KD_MESH: no KDMesh walker compiled in) at 4; with KDMesh trees the kernel needs its 168 registers.
        a.four_waves = c->spawns ? 0 : ((a.scene.mode == PT_MODE_KD_NOMESH && a.scene.n_nodes >= 256) ? 5 : (a.scene.mode == PT_MODE_KD_MESH ? 4 : 0));
        if (const char* e = getenv("PORTRAYER_KD_WAVES")) {
            const int wv = atoi(e);
            a.four_waves = (c->spawns || wv < 4 || a.scene.mode == PT_MODE_KD) ? 0 : ((wv >= 5 && a.scene.mode == PT_MODE_KD_NOMESH) ? 5 : 4);
        }
    }
    // Fork / join of refracted subtrees (pt_shade.h) is built, parity-green and OFF by default: it fills the idle lanes and still loses
    // (transmission-refraction 11.4 -> 8.6 Gray/s, profiles/r03/notes.md section 4): the subtrees other lanes walk are other rays, and the
    // one walk per wavefront pays for the union of their paths. PORTRAYER_FORK=1 switches it on for scenes that qualify.
    bool fork = false;
    if (const char* e = getenv("PORTRAYER_FORK")) fork = c->forkable && a.park_slots && atoi(e) > 0;
    if (c->launch_seq == 0) c->launch_seq = (uint32_t)std::chrono::steady_clock::now().time_since_epoch().count() * 2654435761u;  // a different starting point in every context
    a.launch_nonce = ++c->launch_seq;
    bool chain = c->one_ray;
    if (const char* e = getenv("PORTRAYER_CHAIN")) chain = chain && atoi(e) > 0;  // 0: the interpreter kernel also for scenes whose recursion is a chain (A/B runs, tests)
    if (c->spawns) a.run_variant = (chain && a.park_slots) ? PT_RUN_CHAIN : (a.park_slots ? (fork ? PT_RUN_INTERP_FORK : PT_RUN_INTERP_PARK) : PT_RUN_INTERP);
    else a.run_variant = a.four_waves >= 5 ? PT_RUN_LINE5 : (a.four_waves ? PT_RUN_LINE4 : PT_RUN_LINE3);  // (LINE5: the densest instantiation the mode has)
    if (a.run_variant == PT_RUN_CHAIN) {
        a.park_slots = 0;  // no frame in LDS: the parked colours go straight to the lane's HBM lines
        // 4 waves per SIMD in the flat_scene semantics (mirror scene 25.5 -> 26.8 Gray/s, c34: ten bounces per sample leave a lot of latency to hide),
        // 3 in the hierarchical ones (182 spilled registers at 128: 19.3 -> 14.8) and the k-d ones. PORTRAYER_CHAIN_WAVES=3|4 overrides.
        // (Only where that was measured or the compiler's figures are like the measured case's: untextured, no KDMesh trees - those
        // instantiations spill 57 / 142 registers at 128.)
        const bool flat_sem = (a.scene.mode == PT_MODE_FLAT || a.scene.mode == PT_MODE_FLAT_NOMESH || a.scene.mode == PT_MODE_HIER_MESH) && !tex;  // (HIER_MESH: 22.2 -> 24.2, c41)
        a.four_waves = flat_sem ? 4 : 0;
        if (const char* e = getenv("PORTRAYER_CHAIN_WAVES")) a.four_waves = (atoi(e) == 4 && a.scene.mode != PT_MODE_KD) ? 4 : 0;
        else if (a.scene.mode == PT_MODE_KD_MESH && !tex) a.four_waves = 4;
    }
    size_t block_budget = a.four_waves >= 6 ? 26 * 1024 : (a.four_waves == 5 ? 31 * 1024 : (a.four_waves ? 39 * 1024 : 52 * 1024));  // 3 x 52 KB, 4 x 39 KB, 5 x 31 KB or 6 x 26 KB of the CU's 160 KB
    if (const char* e = getenv("PORTRAYER_LDS_BUDGET_KB")) block_budget = (size_t)std::max(16, std::min(160, atoi(e))) * 1024;  // experiment: 80 = two blocks per CU
    const size_t frame_bytes = (size_t)(PT_LDS_FRAME_F64 + a.park_slots * PT_PARK_F64) * PT_BLOCK * 8;
    a.stack_lds_cap = pt_stack_lds_cap(a.scene, block_budget, frame_bytes);
    a.grid_share = 1;  // (a share of the resident blocks per launch was tried for ranks that share a GPU, round 5 c23: their kernels do not run side by side - 35.5 -> 14.3 Gray/s)
    uint32_t grid = 0;
    PT_HIP(c, pt_dispatch(a, stats, c->n_cu, stream, &grid, false));
    a.n_lanes = grid * PT_BLOCK;
    a.work_div = std::max<uint32_t>(grid * (PT_BLOCK / 64) * 8u, 1u);  // batch = remaining items / (8 x resident wavefronts)
    // How the work items are handed out (pt_render_kernel): batches of consecutive items from one counter, or - scenes whose
    // hits can spawn rays, where an item in the glass costs hundreds of times its neighbour - one item at a time from
    // interleaved queues. transmission-refraction: wavefronts resident 47 % of the launch and 5.2 Gray/s with batches, 11+ without.
    a.batch_max = PT_WORK_BATCH_MAX;
    if (const char* e = getenv("PORTRAYER_BATCH_MAX")) a.batch_max = (uint32_t)std::max(1, atoi(e));
    // The queues also win wherever a wavefront gets few items (a small frame, one GPU's share of a frame: big-scene's 1/8 share +8 %,
    // macho-cows +13 %) and on the mesh-heavy scenes (+3-7 %); very long launches (> 2048 items per resident wavefront: 3840x2160x256)
    // are 1 % better off with batches.
    const uint64_t resident_waves = (uint64_t)grid * (PT_BLOCK / 64);
    const bool long_launch = (uint64_t)a.n_items > 2048ull * std::max<uint64_t>(resident_waves, 1);
    // (round 3's per-lane k-d walk was 1 % better off with batches; the wave-uniform one is not: big-scene +1.1 %, macho-cows +3.2 % with the queues, round 4 c68)
    a.fine_queues = (c->spawns || !long_launch) ? 16 : 0;  // 8 .. 32 queues measured alike, 64 and 4 about 1 % behind
    if (const char* e = getenv("PORTRAYER_FINE_QUEUES")) a.fine_queues = (uint32_t)std::max(0, std::min(PT_FINE_QUEUES, atoi(e)));
    a.item_stride = 1;
    if (const char* e = getenv("PORTRAYER_ITEM_STRIDE")) {  // experiment (batches only): position q -> item (q * stride) mod n; "golden" = 0.618 n
        uint64_t st = strcmp(e, "golden") == 0 ? (uint64_t)((double)a.n_items * 0.6180339887498949) : (uint64_t)atoll(e);
        auto gcd = [](uint64_t x, uint64_t y) { while (y) { uint64_t t = x % y; x = y; y = t; } return x; };
        if (a.n_items > 2 && st != 1) { st = st % a.n_items; if (st < 1) st = 1; while (gcd(st, a.n_items) != 1) st++; a.item_stride = (uint32_t)st; }
    }
    int rc;
    if (slot_index < 0) {  // the host-buffer path (pt_render): one frame at a time
        if (c->slot[c->slot_oldest].pending) return pt_fail(c, PT_ERR_ARGUMENT, "a render is in flight: pt_render_finish first");
        slot_index = c->slot_next;
    }
    pt_context::Slot& sl = c->slot[slot_index];  // the launch's work buffers are its slot's: another frame may be in flight on the other slot's
    const size_t spill_bytes = c->needs_spill ? (size_t)a.n_lanes * PT_SPILL_DEPTHS * PT_SPILL_STRIDE * sizeof(double) : 16;
    if ((rc = pt_reserve(c, sl.spill, spill_bytes))) return rc;
    const size_t stack_column = pt_stack_column(a.scene, a.stack_lds_cap);
    if ((rc = pt_reserve(c, sl.stack_spill, (size_t)a.n_lanes * stack_column * 4))) return rc;  // (the k-d walk's saved bounds needed columns behind this until round 5)
    // The occluder table of the mesh-free walks' shadow rays (pt_trace_packet): one word per (own 8x8 tile, light), behind the work
    // queues, zeroed with them before every launch - what it remembers comes from the frame being rendered, never from an earlier one.
    // PORTRAYER_SHADOW_CACHE=0 leaves it out (A/B runs); so does a table of more than 4 MB (many lights: zeroing it would cost more).
    const size_t misc_head = 256 + sizeof(PtCounters) + PT_FINE_QUEUES * PT_QUEUE_STRIDE * 4;
    size_t occ_bytes = (size_t)(a.n_slots / 64) * a.scene.n_lights * 4;
    if (!(a.scene.mode == PT_MODE_FLAT_NOMESH || a.scene.mode == PT_MODE_HIER_NOMESH) || occ_bytes > ((size_t)4 << 20)) occ_bytes = 0;
    if (const char* e = getenv("PORTRAYER_SHADOW_CACHE")) if (atoi(e) <= 0) occ_bytes = 0;
    // PORTRAYER_OCC_SEED=all:K | <seed> (tests only): the table starts with hints the test chose (pt_occ_seed_kernel), not with zeros
    bool occ_seed = false, occ_hashed = false;
    uint64_t occ_seed_value = 0;
    uint32_t occ_all = 0;
    if (const char* e = getenv("PORTRAYER_OCC_SEED"); e && *e && occ_bytes) {
        char* end = nullptr;
        if (strncmp(e, "all:", 4) == 0) {
            const unsigned long long k = strtoull(e + 4, &end, 10);
            if (end == e + 4 || *end || k >= a.scene.n_nodes) return pt_fail(c, PT_ERR_ARGUMENT, std::string("PORTRAYER_OCC_SEED=") + e + ": K must be a node index below " + std::to_string(a.scene.n_nodes));
            occ_all = (uint32_t)k;
        } else {
            occ_seed_value = strtoull(e, &end, 10);
            if (end == e || *end) return pt_fail(c, PT_ERR_ARGUMENT, std::string("PORTRAYER_OCC_SEED=") + e + ": expected all:<node> or a decimal seed");
            occ_hashed = true;
        }
        occ_seed = true;
    }
    if ((rc = pt_reserve(c, sl.misc, misc_head + occ_bytes))) return rc;
    if ((rc = pt_reserve(c, sl.accum, (size_t)a.n_slots * a.n_chunks * 3 * sizeof(double)))) return rc;
    a.accum = (double*)sl.accum.p;
    // The eye table of the mesh-free flat_scene semantics (pt_render_simple.h: EYE_TABLE): every launch in that mode gets one, whichever kernel runs - the counting,
    // chain and interpreter kernels do not read it, and a launch's choice of kernel must never leave a kernel that does without
#ifndef PT_NO_EYE_TABLE
    const bool eye_table = a.scene.mode == PT_MODE_FLAT_NOMESH && a.scene.n_nodes > 0;
#else
    const bool eye_table = false;
#endif
    // The certain-shadow table (pt_render_simple.h: CERTAIN) behind it: the flat_scene launches that have an occluder table, whichever kernel runs
#ifndef PT_NO_CERTAIN_SHADOW
    const bool certain_table = a.scene.mode == PT_MODE_FLAT_NOMESH && a.scene.n_nodes > 0 && occ_bytes != 0;
#else
    const bool certain_table = false;
#endif
    // The per-pixel candidate lists (pt_pixel_list.h; pt_render_simple.h: PIXEL_LISTS) behind both: the launches whose kernel reads them - the plain straight-line kernels of
    // this mode where a wavefront is one pixel - and scenes whose node indices fit an entry's 16 bits. Their 64-byte header is written in every launch that has an eye table
    // (0: no lists). PORTRAYER_PIXEL_LISTS=0: none (the walk's image from the same library); PORTRAYER_PIXEL_LIST_CAP=k (tests only): a list holds k entries at most, so that
    // small scenes reach the tail bound and the fall-back. -DPT_NO_PIXEL_LISTS: no header, no lists, the kernels as they were (A/B).
#ifndef PT_NO_PIXEL_LISTS
    const bool list_header = eye_table;
#ifdef PT_PIXEL_LIST_STATS  // the counting build evaluates the lists beside its walk (pt_render_simple.h): it gets them too
    const bool list_reader = true;
#else
    const bool list_reader = !stats;
#endif
    bool pixel_lists = eye_table && list_reader && (a.run_variant == PT_RUN_LINE3 || a.run_variant == PT_RUN_LINE4 || a.run_variant == PT_RUN_LINE5) && a.k_log2 + a.c_log2 == 6u &&
                       a.scene.n_nodes <= PT_PL_MAX_NODES && a.n_slots != 0;
    if (const char* e = getenv("PORTRAYER_PIXEL_LISTS")) if (atoi(e) <= 0) pixel_lists = false;
    uint32_t list_cap = PT_PL_K;
    if (const char* e = getenv("PORTRAYER_PIXEL_LIST_CAP"); e && *e) {
        char* end = nullptr;
        const unsigned long long k = strtoull(e, &end, 10);
        if (end == e || *end || k > PT_PL_K) return pt_fail(c, PT_ERR_ARGUMENT, std::string("PORTRAYER_PIXEL_LIST_CAP=") + e + ": expected 0 .. " + std::to_string(PT_PL_K));
        list_cap = (uint32_t)k;
    }
#else
    const bool list_header = false, pixel_lists = false;
    const uint32_t list_cap = 0;
#endif
    const size_t list_off = pt_pl_header_offset((uint32_t)a.scene.n_nodes);
    a.eye_tab = nullptr;
    if (eye_table || certain_table) {
        if ((rc = pt_reserve(c, sl.eye_tab, list_header ? list_off + pt_pl_bytes(pixel_lists ? a.n_slots : 0u) : (size_t)a.scene.n_nodes * (12 * sizeof(double) + 4 * sizeof(float))))) return rc;
        a.eye_tab = (const double*)sl.eye_tab.p;
    }
    a.spill = (double*)sl.spill.p;
    a.stack_spill = (uint32_t*)sl.stack_spill.p;
    a.work_counter = (unsigned int*)sl.misc.p;
    a.overflow_flag = (unsigned int*)sl.misc.p + 1;
    a.counters = (PtCounters*)((char*)sl.misc.p + 256);
    a.work_queues = (unsigned int*)((char*)sl.misc.p + 256 + sizeof(PtCounters));
    a.occluders = occ_bytes ? (uint32_t*)((char*)sl.misc.p + misc_head) : nullptr;
    a.occ_row = std::max<uint32_t>(a.div_tiles_x.d / std::max<uint32_t>(a.tile_ranks, 1u), 1u);
    c->last_mode = (uint32_t)a.scene.mode;
    c->last_variant = (a.four_waves ? (uint32_t)a.four_waves : 3u) | ((a.run_variant == PT_RUN_LINE3 || a.run_variant == PT_RUN_LINE4 || a.run_variant == PT_RUN_LINE5 || a.run_variant == PT_RUN_CHAIN) ? 0u : PT_KERNEL_INTERPRETER) | (a.run_variant == PT_RUN_CHAIN ? PT_KERNEL_CHAIN : 0u) |
                      ((a.run_variant == PT_RUN_INTERP_PARK || a.run_variant == PT_RUN_INTERP_FORK) ? PT_KERNEL_PARK : 0u) | (a.run_variant == PT_RUN_INTERP_FORK ? PT_KERNEL_FORK : 0u) | (stats ? PT_KERNEL_COUNTING : 0u) | (tex ? PT_KERNEL_TEXTURED : 0u);
    PT_HIP(c, hipMemsetAsync(sl.misc.p, 0, misc_head + occ_bytes, stream));
    if (occ_seed) {
        const uint32_t n_occ = (uint32_t)(occ_bytes / 4);
        hipLaunchKernelGGL(pt_occ_seed_kernel, dim3((n_occ + 255) / 256), dim3(256), 0, stream, a.occluders, n_occ, occ_hashed ? 1 : 0, occ_seed_value, occ_all, a.scene.n_nodes);
        PT_HIP(c, hipGetLastError());
        if (getenv("PORTRAYER_VERBOSE")) fprintf(stderr, "[pt_render] occluder table: %u entries seeded (PORTRAYER_OCC_SEED=%s)\n", n_occ, getenv("PORTRAYER_OCC_SEED"));
    }
    sl.mode = c->last_mode; sl.variant = c->last_variant; sl.counted = stats;
    PT_HIP(c, hipEventRecord(sl.ev0, stream));
    if (a.n_items) {
        if (eye_table) {  // (behind ev0: pt_stats.kernel_ms pays for it)
            hipLaunchKernelGGL(pt_eye_table_kernel, dim3((a.scene.n_nodes + 255) / 256), dim3(256), 0, stream, a.scene.inv, (double*)sl.eye_tab.p, (uint32_t)a.scene.n_nodes,
                               a.cam.eye[0], a.cam.eye[1], a.cam.eye[2]);
            PT_HIP(c, hipGetLastError());
        }
        if (certain_table) {
            hipLaunchKernelGGL(pt_certain_table_kernel, dim3((a.scene.n_nodes + 255) / 256), dim3(256), 0, stream, a.scene.info, a.scene.fwd, a.scene.inv, (float*)((double*)sl.eye_tab.p + 12 * (size_t)a.scene.n_nodes),
                               (uint32_t)a.scene.n_nodes);
            PT_HIP(c, hipGetLastError());
        }
        if (list_header) {  // behind the eye table's fill, on the launch's stream: the header, then the slot's records
            uint32_t* const header = (uint32_t*)((char*)sl.eye_tab.p + list_off);
            PT_HIP(c, hipMemsetD32Async((hipDeviceptr_t)header, pixel_lists ? 1 : 0, 16, stream));
            if (pixel_lists) {
                const uint32_t tiles = a.n_slots / 64u;
                hipLaunchKernelGGL(pt_pixel_list_kernel, dim3((tiles + PT_PL_BLOCK / 64 - 1) / (PT_PL_BLOCK / 64)), dim3(PT_PL_BLOCK), 0, stream, a, header + 16, list_cap);
                PT_HIP(c, hipGetLastError());
            }
        }
        c->pl_slot = pixel_lists ? slot_index : -1; c->pl_slots = a.n_slots; c->pl_off = list_off + 64;
        PT_HIP(c, pt_dispatch(a, stats, c->n_cu, stream, &grid, true));
        hipLaunchKernelGGL(pt_finish_kernel, dim3((a.n_slots + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), 0, stream, a);
        PT_HIP(c, hipGetLastError());
    }
    PT_HIP(c, hipEventRecord(sl.ev1, stream));
    // the overflow flag (always) and the counters (counting build) follow the kernels into the slot's pinned page
    PT_HIP(c, hipMemcpyAsync(sl.host, sl.misc.p, stats ? PT_SLOT_BYTES : 8, hipMemcpyDeviceToHost, stream));
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

// What refuses a second pass on the pass object pt_aov and pt_guides share: the open one's kind and the call that closes it.
static const char* pt_aov_open_words(const pt_context* c) {
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
    void* host[6] = {host_out->depth, host_out->position, host_out->normal, host_out->node, host_out->sub, host_out->material};
    const size_t elem[6] = {8, 24, 24, 4, 4, 4};  // bytes per pixel
    void* dev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < 6; k++) {
        if (!host[k]) continue;
        if ((rc = pt_reserve(c, c->aov.out[k], px * elem[k]))) return rc;
        dev[k] = c->aov.out[k].p;
    }
    pt_aov_buffers d_out;
    d_out.depth = (double*)dev[0]; d_out.position = (double*)dev[1]; d_out.normal = (double*)dev[2];
    d_out.node = (int32_t*)dev[3]; d_out.sub = (int32_t*)dev[4]; d_out.material = (int32_t*)dev[5];
    if ((rc = pt_pass_settle(c, c->aov.pass, pt_aov_common(c, cam, p, d_out, nullptr)))) return rc;
    // Only the slice's rectangle comes back (the kernel wrote nothing else, and the device copies hold nothing else of value): picking one pixel of a
    // 1920x1080 frame moves 68 bytes, and pixels outside the slice keep the caller's bytes because they are never touched.
    if (p->slice.x1 >= p->slice.x0 && p->slice.y1 >= p->slice.y0) {
        const size_t cols = (size_t)p->slice.x1 - p->slice.x0 + 1, rows = (size_t)p->slice.y1 - p->slice.y0 + 1;
        for (int k = 0; k < 6; k++) {
            if (!host[k]) continue;
            const size_t pitch = (size_t)p->width * elem[k], first = ((size_t)p->slice.y0 * p->width + p->slice.x0) * elem[k];
            PT_HIP(c, hipMemcpy2D((char*)host[k] + first, pitch, (const char*)dev[k] + first, pitch, cols * elem[k], rows, hipMemcpyDeviceToHost));
        }
    }
    return pt_pass_result(c, c->aov.pass, kernel_ms);
}

extern "C" int pt_aov_device(pt_context* c, const pt_camera* cam, const pt_aov_params* p, const pt_aov_buffers* device_out, void* hip_stream) {
    int rc = pt_aov_check(c, cam, p, device_out);
    if (rc) return rc;
    PT_HIP(c, hipSetDevice(c->device));
    c->aov.guides = false;
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
    void* host[4] = {host_out->albedo, host_out->position, host_out->normal, host_out->node};
    PtBuf* buf[4] = {&c->aov.albedo, &c->aov.out[1], &c->aov.out[2], &c->aov.out[3]};
    const size_t elem[4] = {24, 24, 24, 4};  // bytes per pixel
    void* dev[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < 4; k++) {
        if (!host[k]) continue;
        if ((rc = pt_reserve(c, *buf[k], px * elem[k]))) return rc;
        dev[k] = buf[k]->p;
    }
    pt_guides_buffers d_out;
    d_out.albedo = (double*)dev[0]; d_out.position = (double*)dev[1]; d_out.normal = (double*)dev[2]; d_out.node = (int32_t*)dev[3];
    if ((rc = pt_pass_settle(c, c->aov.pass, pt_guides_common(c, cam, p, d_out, nullptr)))) return rc;
    // only the slice's rectangle comes back, as in pt_aov: pixels outside it keep the caller's bytes
    if (p->slice.x1 >= p->slice.x0 && p->slice.y1 >= p->slice.y0) {
        const size_t cols = (size_t)p->slice.x1 - p->slice.x0 + 1, rows = (size_t)p->slice.y1 - p->slice.y0 + 1;
        for (int k = 0; k < 4; k++) {
            if (!host[k]) continue;
            const size_t pitch = (size_t)p->width * elem[k], first = ((size_t)p->slice.y0 * p->width + p->slice.x0) * elem[k];
            PT_HIP(c, hipMemcpy2D((char*)host[k] + first, pitch, (const char*)dev[k] + first, pitch, cols * elem[k], rows, hipMemcpyDeviceToHost));
        }
    }
    return pt_pass_result(c, c->aov.pass, kernel_ms);
}

extern "C" int pt_guides_device(pt_context* c, const pt_camera* cam, const pt_aov_params* p, const pt_guides_buffers* device_out, void* hip_stream) {
    int rc = pt_guides_check(c, cam, p, device_out);
    if (rc) return rc;
    PT_HIP(c, hipSetDevice(c->device));
    c->aov.guides = true;
    return pt_pass_device_tail(c, c->aov.pass, pt_guides_common(c, cam, p, *device_out, (hipStream_t)hip_stream));
}

// The pass is pt_aov's: one function closes either.
extern "C" int pt_guides_finish(pt_context* c, double* kernel_ms) { return pt_aov_finish(c, kernel_ms); }

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
    void* host[7] = {host_out->t, host_out->position, host_out->normal, host_out->node, host_out->sub, host_out->material, host_out->occluded};
    const size_t elem[7] = {8, 24, 24, 4, 4, 4, 1};  // bytes per ray
    void* dev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int rc;
    if ((rc = pt_reserve(c, c->rays.in[0], n * 24)) || (rc = pt_reserve(c, c->rays.in[1], n * 24))) return rc;
    if (t_max && (rc = pt_reserve(c, c->rays.in_t_max, n * 8))) return rc;
    for (int k = 0; k < 7; k++) {
        if (!host[k]) continue;
        if ((rc = pt_reserve(c, c->rays.out[k], n * elem[k]))) return rc;
        dev[k] = c->rays.out[k].p;
    }
    PT_HIP(c, hipMemcpy(c->rays.in[0].p, origins, n * 24, hipMemcpyHostToDevice));
    PT_HIP(c, hipMemcpy(c->rays.in[1].p, directions, n * 24, hipMemcpyHostToDevice));
    if (t_max) PT_HIP(c, hipMemcpy(c->rays.in_t_max.p, t_max, n * 8, hipMemcpyHostToDevice));
    pt_rays_buffers d_out;
    d_out.t = (double*)dev[0]; d_out.position = (double*)dev[1]; d_out.normal = (double*)dev[2];
    d_out.node = (int32_t*)dev[3]; d_out.sub = (int32_t*)dev[4]; d_out.material = (int32_t*)dev[5]; d_out.occluded = (uint8_t*)dev[6];
    rc = pt_rays_common(c, p, (const double*)c->rays.in[0].p, (const double*)c->rays.in[1].p, d_out, nullptr, t_max ? (const double*)c->rays.in_t_max.p : nullptr);
    if ((rc = pt_pass_settle(c, c->rays.pass, rc))) return rc;
    for (int k = 0; k < 7; k++)
        if (host[k]) PT_HIP(c, hipMemcpy(host[k], dev[k], n * elem[k], hipMemcpyDeviceToHost));
    return pt_pass_result(c, c->rays.pass, kernel_ms);
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

static PtAoSet pt_ao_set(const pt_ao_params* p) {
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
    a.r.stack_lds_cap = pt_stack_lds_cap(a.r.scene, pt_ao_waves(a.r.scene.mode) == 3 ? 52 * 1024 : 39 * 1024, pt_ao_frame_bytes(layout));  // (pt_walk_sizing's budgets)
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
    void* host[3] = {host_out->occluded, host_out->valid, host_out->bent};
    PtBuf* buf[3] = {&c->rays.out[3], &c->rays.out[6], &c->rays.out[1]};
    const size_t elem[3] = {4, 1, 24};  // bytes per point
    void* dev[3] = {nullptr, nullptr, nullptr};
    if ((rc = pt_reserve(c, c->rays.in[0], n * 24)) || (rc = pt_reserve(c, c->rays.in[1], n * 24))) return rc;
    for (int k = 0; k < 3; k++) {
        if (!host[k]) continue;
        if ((rc = pt_reserve(c, *buf[k], n * elem[k]))) return rc;
        dev[k] = buf[k]->p;
    }
    PT_HIP(c, hipMemcpy(c->rays.in[0].p, positions, n * 24, hipMemcpyHostToDevice));
    PT_HIP(c, hipMemcpy(c->rays.in[1].p, normals, n * 24, hipMemcpyHostToDevice));
    pt_ao_buffers d_out;
    d_out.occluded = (uint32_t*)dev[0]; d_out.valid = (uint8_t*)dev[1]; d_out.bent = (double*)dev[2];
    rc = pt_ao_common(c, p, (const double*)c->rays.in[0].p, (const double*)c->rays.in[1].p, d_out, nullptr);
    if ((rc = pt_pass_settle(c, c->rays.pass, rc))) return rc;
    for (int k = 0; k < 3; k++)
        if (host[k]) PT_HIP(c, hipMemcpy(host[k], dev[k], n * elem[k], hipMemcpyDeviceToHost));
    return pt_pass_result(c, c->rays.pass, kernel_ms);
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
    if ((rc = pt_reserve(c, v.in[0], n * 24)) || (rc = pt_reserve(c, v.in[1], n * 24)) || (rc = pt_reserve(c, v.in[2], bg_bytes)) || (rc = pt_reserve(c, v.out, n * 24))) return rc;
    PT_HIP(c, hipMemcpy(v.in[0].p, origins, n * 24, hipMemcpyHostToDevice));
    PT_HIP(c, hipMemcpy(v.in[1].p, directions, n * 24, hipMemcpyHostToDevice));
    PT_HIP(c, hipMemcpy(v.in[2].p, background, bg_bytes, hipMemcpyHostToDevice));
    rc = pt_radiance_common(c, p, (const double*)v.in[0].p, (const double*)v.in[1].p, (const double*)v.in[2].p, (double*)v.out.p, nullptr);
    if ((rc = pt_pass_settle(c, v.pass, rc))) return rc;
    PT_HIP(c, hipMemcpy(rgb, v.out.p, n * 24, hipMemcpyDeviceToHost));
    return pt_pass_result(c, v.pass, kernel_ms);
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
    // what steps 1 to 8 read (pt_ao_set: the eye only with PT_AO_FACE_EYE)
    a.set.seed = p->seed; a.set.first_index = p->first_index; a.set.pass = p->pass; a.set.flags = p->flags; a.set.bias = p->bias;
    a.set.eye = (p->flags & PT_AO_FACE_EYE) ? pt_v3(p->eye[0], p->eye[1], p->eye[2]) : pt_v3(0.0, 0.0, 0.0);
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
    if ((rc = pt_reserve(c, v.in[0], n * 24)) || (rc = pt_reserve(c, v.in[1], n * 24))) return rc;
    if (host_out->sum && (rc = pt_reserve(c, v.out, n * 24))) return rc;
    if (host_out->valid && (rc = pt_reserve(c, v.in[2], n))) return rc;
    PT_HIP(c, hipMemcpy(v.in[0].p, positions, n * 24, hipMemcpyHostToDevice));
    PT_HIP(c, hipMemcpy(v.in[1].p, normals, n * 24, hipMemcpyHostToDevice));
    pt_gather_buffers d_out;
    d_out.sum = host_out->sum ? (double*)v.out.p : nullptr;
    d_out.valid = host_out->valid ? (uint8_t*)v.in[2].p : nullptr;
    rc = pt_gather_common(c, p, (const double*)v.in[0].p, (const double*)v.in[1].p, background, d_out, nullptr);
    if ((rc = pt_pass_settle(c, v.pass, rc))) return rc;
    if (host_out->sum) PT_HIP(c, hipMemcpy(host_out->sum, d_out.sum, n * 24, hipMemcpyDeviceToHost));
    if (host_out->valid) PT_HIP(c, hipMemcpy(host_out->valid, d_out.valid, n, hipMemcpyDeviceToHost));
    return pt_pass_result(c, v.pass, kernel_ms);
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
// Film: samples accumulate on the device (pt_film.h, pt_film.hip)
// ------------------------------------------------------------------------------------------------
static hipError_t pt_film_dispatch(const PtFilmArgs& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    PT_MODE_LAUNCH(pt_film_launch_mode_, a.r.scene.mode, a, tex, park, n_cu, stream, grid, launch)
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
    if (!c || !f || !cam || !background || !p) return pt_fail(c, PT_ERR_ARGUMENT, "pt_film_add: NULL context, film, camera, background or params");
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

static int pt_film_add_common(pt_context* c, pt_film* f, const pt_camera* cam, const double* d_background, const pt_film_params* p, hipStream_t stream) {
    PtPass& v = c->radiance.pass;
    uint32_t lw = PT_FILM_LW;
    if (const char* e = getenv("PORTRAYER_FILM_LW")) { const int w = atoi(e); if (w == 8 || w == 64) lw = (uint32_t)w; }  // measurements (profiles/film)
    if (f->moments) lw = PT_FILM_LW;  // (the fold that keeps q takes at most PT_FILM_LW samples per launch: pt_film_map_round)
    PtFilmArgs a;
    PtInterp k;
    int rc = pt_film_pass_args(c, f, cam, d_background, p->slice, p->seed, p->sample_mode, p->background_rows, lw, a, k);
    if (rc) return rc;
    const uint32_t tiles = a.r.n_slots / 64u;
    // the buffers are sized for the add's largest launch (its first: min(samples, lw) samples per pixel); the later ones use a prefix of the same lanes
    auto set_launch = [&](uint32_t m) {
        a.launch_samples = m;
        for (a.k_log2 = 0; (1u << a.k_log2) < m; a.k_log2++) { }
        a.r.n_items = tiles << a.k_log2;  // (tiles < 2^25, K <= 64)
    };
    set_launch(std::min(p->samples, lw));
    uint32_t grid = 0;
    PT_HIP(c, pt_film_dispatch(a, k.tex, k.park, c->n_cu, stream, &grid, false));
    if ((rc = pt_reserve(c, f->staging, (size_t)a.r.n_slots * a.lw * 24))) return rc;
    a.staging = (double*)f->staging.p;
    if ((rc = pt_pass_open(c, v, a.r, grid, true, stream))) return rc;
    for (uint32_t left = p->samples, first = 1; left > 0; first = 0) {
        const uint32_t m = std::min(left, lw);
        set_launch(m);
        if (!first) PT_HIP(c, hipMemsetAsync((char*)v.misc.p + 256, 0, PT_PASS_MISC_BYTES - 256, stream));  // the queues again; the overflow flag stays
        uint32_t g = 0;
        PT_HIP(c, pt_film_dispatch(a, k.tex, k.park, c->n_cu, stream, &g, true));  // (g <= grid: no more items than the launch the buffers were sized for)
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

extern "C" int pt_film_add(pt_context* c, pt_film* f, const pt_camera* cam, const double* background, const pt_film_params* p, double* kernel_ms) {
    int rc = pt_film_add_check(c, f, cam, background, p);
    if (rc) return rc;
    if (kernel_ms) *kernel_ms = 0.0;
    if (pt_film_slice_empty(p)) return PT_OK;
    PT_HIP(c, hipSetDevice(c->device));
    const size_t bg_bytes = (p->background_rows ? (size_t)f->height : (size_t)f->height * f->width) * 24;
    if ((rc = pt_reserve(c, f->bg, bg_bytes))) return rc;
    PT_HIP(c, hipMemcpy(f->bg.p, background, bg_bytes, hipMemcpyHostToDevice));
    if ((rc = pt_pass_settle(c, c->radiance.pass, pt_film_add_common(c, f, cam, (const double*)f->bg.p, p, nullptr)))) return rc;
    return pt_pass_result(c, c->radiance.pass, kernel_ms);
}

extern "C" int pt_film_add_device(pt_context* c, pt_film* f, const pt_camera* cam, const double* d_background, const pt_film_params* p, void* hip_stream) {
    int rc = pt_film_add_check(c, f, cam, d_background, p);
    if (rc) return rc;
    if (pt_film_slice_empty(p)) return PT_OK;  // nothing queued, nothing to finish
    PT_HIP(c, hipSetDevice(c->device));
    if ((rc = pt_pass_device_tail(c, c->radiance.pass, pt_film_add_common(c, f, cam, d_background, p, (hipStream_t)hip_stream)))) return rc;
    c->film_open = f;
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
    bool tiled = true;  // the LDS-tiled form, the faster one at 5 levels by more than three spreads (profiles/denoise/notes.md), unless the switch says otherwise
    if (const char* e = getenv("PORTRAYER_DENOISE_TILE")) tiled = atoi(e) > 0;
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
            if (getenv("PORTRAYER_VERBOSE")) fprintf(stderr, "[pt_measure_copy_bandwidth] form %d: %.0f GB/s\n", form, rate);
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
