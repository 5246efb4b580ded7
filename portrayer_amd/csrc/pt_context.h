// What the units behind the C ABI share (pt_api.hip: the context's life cycle, the render and the passes; pt_scene.hip: scene upload, update and deform): the
// context itself, device buffers, the error helpers. Internal: nothing outside portrayer_amd/csrc includes this.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/portrayer_hip.h"
#include "pt_build.h"
#include "pt_bvh.h"
#include "pt_shade.h"

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

// What an uploaded scene says (include/portrayer_hip.h) and the three things the recursion's shape follows from:
typedef pt_scene_traits PtSceneTraits;
// some material is reflective: hits spawn rays, so the cost of a pixel varies by orders of magnitude
static bool pt_spawns(const PtSceneTraits& t) { return t.reflective != 0; }
// some material is reflective (recursion frames) or the scene has more than 32 lights: the lanes keep frames in HBM
static bool pt_needs_spill(const PtSceneTraits& t) { return pt_spawns(t) || t.n_lights > PT_LIGHT_ROUND; }

// the mode pt_scene_upload gives a scene: the general walker (meshes and KDMesh trees compiled in), or its instantiation without KDMesh trees, or the mesh-free one
static int pt_scene_mode(const PtSceneTraits& t) {
    if (t.traverse == PT_TRAVERSE_KD) return !t.has_meshes ? PT_MODE_KD_NOMESH : (t.has_kdmesh ? PT_MODE_KD : PT_MODE_KD_MESH);
    if (t.traverse == PT_TRAVERSE_HIER) return !t.has_meshes ? PT_MODE_HIER_NOMESH : (t.has_kdmesh ? PT_MODE_HIER : PT_MODE_HIER_MESH);
    return !t.has_meshes ? PT_MODE_FLAT_NOMESH : (t.has_kdmesh ? PT_MODE_FLAT_KDMESH : PT_MODE_FLAT);
}

// ------------------------------------------------------------------------------------------------
// Environment switches (PORTRAYER_*), read at every launch - tests flip them between launches of one process - in three forms.
// ------------------------------------------------------------------------------------------------
// Set at all, whatever to (experiments, PORTRAYER_VERBOSE).
static bool pt_env_set(const char* name) { return getenv(name) != nullptr; }
// On / off: unset -> `unset`; set -> on exactly where atoi() of it is positive ("0", "", words: off).
static bool pt_env_on(const char* name, bool unset) {
    const char* e = getenv(name);
    return e ? atoi(e) > 0 : unset;
}
// A lenient integer: unset -> `unset`; set -> atoi() of it, clamped to lo .. hi.
static int pt_env_clamped(const char* name, int unset, int lo, int hi) {
    const char* e = getenv(name);
    return e ? std::max(lo, std::min(hi, atoi(e))) : unset;
}
// A strict unsigned integer: unset or empty -> true, *value untouched; all of it a decimal number in lo .. hi -> true, *value set; anything else -> false and
// *why = "NAME=text: expected lo .. hi".
static bool pt_env_strict(const char* name, unsigned long long lo, unsigned long long hi, uint32_t* value, std::string* why) {
    const char* e = getenv(name);
    if (!e || !*e) return true;
    char* end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (end == e || *end || v < lo || v > hi) {
        *why = std::string(name) + "=" + e + ": expected " + std::to_string(lo) + " .. " + std::to_string(hi);
        return false;
    }
    *value = (uint32_t)v;
    return true;
}
// PORTRAYER_PARK=0: every parked recursion frame in HBM (tests, measurements) - the render's interpreter kernels and the interpreter passes alike
static bool pt_env_park() { return pt_env_on("PORTRAYER_PARK", true); }

// The LDS a block may take where `waves` wavefronts per SIMD are to be resident: a CU has 160 KB, a block is four wavefronts, one per SIMD - 3 x 52 KB, 4 x 39 KB,
// 5 x 31 KB or 6 x 26 KB.
static size_t pt_block_budget(int waves) { return (size_t)(waves >= 6 ? 26 : (waves == 5 ? 31 : (waves == 4 ? 39 : 52))) * 1024; }

// ------------------------------------------------------------------------------------------------
// A render launch as planned (pt_api.hip: pt_choose_kernel, pt_plan_launch) - what pt_render_common commits.
// ------------------------------------------------------------------------------------------------
// Which render kernel a scene runs: PtRenderArgs::run_variant, the waves per SIMD its instantiation is compiled for (PtRenderArgs::four_waves: 0 = three),
// the parked frames kept in LDS and the LDS a block may take.
struct PtKernelChoice {
    int run_variant = PT_RUN_LINE3, four_waves = 0, park_slots = 0;
    size_t block_budget = 0;
    bool needs_spill = false;  // the lanes keep recursion frames in HBM
};
enum PtOccSeed { PT_OCC_SEED_NONE = 0, PT_OCC_SEED_HASHED = 1, PT_OCC_SEED_ALL = 2 };  // PORTRAYER_OCC_SEED: unset, <seed>, all:K
struct PtLaunchPlan {
    PtKernelChoice choice;
    uint32_t kernel_mode = 0, kernel_variant = 0;  // pt_stats' words, PT_KERNEL_COUNTING included
    int stack_lds_cap = 0;
    uint32_t grid_share = 1;
    // how the work items are dealt
    uint32_t n_lanes = 0, work_div = 1, batch_max = 0, fine_queues = 0, item_stride = 1;
    // the slot's buffers, in bytes
    size_t spill = 0, stack_spill = 0, misc = 0, accum = 0, eye_tab = 0;
    //   misc:    [0 work counter, overflow flag | 256 PtCounters | work queues | dark_off: dark-light records | occ_off: occluder table | misc)
    //   eye_tab: [0 eye table | certain_off: certain-shadow table | header_off: list header, 64 bytes | records_off: records | queue_off: queue, tile masks | eye_tab)
    // A region the launch does not have is empty and its offset the next region's.
    size_t dark_off = 0, dark_bytes = 0, occ_off = 0, occ_bytes = 0;
    size_t certain_off = 0, header_off = 0, records_off = 0, queue_off = 0;
    // what the launch has (dark_lights: the kernel that fills the records runs - they are zeroed in any case)
    bool eye_table = false, certain_table = false, dark_lights = false, list_header = false, pixel_lists = false, background_skip = false;
    uint32_t list_cap = 0, list_pending = 0, occ_row = 1;
    uint32_t header_fill = 0;         // the word the list header's 16 are set to in front of the list kernel
    int occ_seed = PT_OCC_SEED_NONE;  // PtOccSeed ...
    uint64_t occ_seed_value = 0;      // ... hashed: the seed ...
    uint32_t occ_all = 0;             // ... all:K: K
    uint32_t n_slots = 0, n_nodes = 0, n_lights = 0;  // what the regions are sized by
};
// What the context's last render launch left behind, for the pt_test_* hooks: its slot (-1: no launch with work items yet) and its plan.
struct PtLastLaunch {
    int slot = -1;
    PtLaunchPlan plan;
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
    PtSceneTraits traits = {};  // what the scene says; what follows from it for a launch: pt_choose_kernel
    uint32_t launch_seq = 0;    // PtRenderArgs::launch_nonce
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
        PtBuf spill, stack_spill, accum, misc;     // misc: work counter + overflow flag (8 B), PtCounters at +256, the work queues behind them, then the dark-light records and the occluder table
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
    PtLastLaunch last;     // what the last render launch left behind (the pt_test_* hooks)
    // The three passes beside the render, each with a PtPass of its own: all three may be in flight at once, with two renders. Beside it, what is the kind's.
    // The primary-visibility pass (pt_aov / pt_aov_device ... pt_aov_finish): the device copies of the host-buffer path's six outputs.
    // The guides pass (pt_guides ...) runs on the SAME pass - one of the two in flight, one set of stack columns - and its host-buffer path takes position, normal and
    // node from out[1 .. 3] and the albedo from a buffer of its own.
    struct Aov {
        PtPass pass;
        PtBuf out[6];
        PtBuf albedo;
        bool guides = false;  // the pass in flight (pass.pending) is a pt_guides_device one: which words a refusal uses
        // The chart pass (pt_chart / pt_chart_device) runs on this pass too: its owner map (4 bytes per texel, grown on demand), and the host-buffer path's
        // device copies of the UV set and of `covered` (position, normal and tri: out[1 .. 3])
        PtBuf chart_owner, chart_uv, chart_covered;
        bool chart = false;   // ... or a pt_chart_device one
    } aov;
    // The ray-query pass (pt_rays / pt_segments, their _device forms ... pt_rays_finish): the device copies of the host-buffer path's inputs (in_t_max: pt_segments'
    // third) and seven outputs.
    struct Rays {
        PtPass pass;
        PtBuf in[2], in_t_max, out[7];
        PtRaySort sort;
    } rays;
    // The radiance pass (pt_radiance / pt_radiance_device ... pt_radiance_finish), which a film's passes share: the device copies of the host-buffer path's three
    // inputs and its output. probe_partial: the probe pass's partial sums between its kernel and its fold (pt_probe_common), at most 32 MiB.
    struct Radiance {
        PtPass pass;
        PtBuf in[3], out;
        PtRaySort sort;
        PtBuf probe_partial;
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
        // pt_scene_deform: where every mesh's tree sits in bvh / bvh4 (nodes) and bvh_items / tri_leaf (items), who built it and how deep it is; the
        // meshes' indices as uploaded (they go to the device with the first deform) and the PtMeshInfo records (bbox_inv and blas_root change)
        struct MeshPlace {
            uint32_t node_first = 0, node_count = 0, item_first = 0, item_count = 0, n_verts = 0;
            int depth = 0;                 // of the two-child tree
            bool device_built = false;     // its place has the device builder's worst-case size: it can be rebuilt there
            bool has_normals = false;
            bool has_uv = false;           // tri_uv holds the mesh's own texture coordinates (a textured scene, mesh_has_texcoords): pt_chart's default UV set
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

// pt_scene.hip: what keeps a caller's device pointer from becoming a GPU fault (the deforms' vertices there, the denoiser's guides in pt_api.hip)
int pt_check_device_pointer(pt_context* c, const void* p, uint64_t bytes, const std::string& what);

