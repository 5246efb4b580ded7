// The render kernel for scenes whose hits spawn no rays (no reflective material: material.rs:216 never takes the branch) -
// render.rs:127-150 and everything below it as ONE straight line per work item, no interpreter:
//
//     primary ray (camera.rs:48-84)  ->  nearest hit  ->  surface + material (flat_scene.rs:85-95, material.rs:109-144)
//     for every light in order (material.rs:149-210):  shadow ray -> any hit ? nothing : colour += (diffuse + specular) / attenuation
//     -> the sample's colour (ray.rs:139-148), summed with its chunk (the summation contract, pt_shade.h)
//
// Without recursion every sample of a work item goes through the same sequence of rays, so the 64 lanes of a wavefront stay in
// step by construction: what pt_lane_advance() (pt_shade.h, still the kernel of reflective scenes) does with a stage word, a
// dispatch loop and a frame in LDS per lane is here plain control flow, and a light's direction and distance are worked out once -
// for the shadow ray - and used again for the shading term (the interpreter recomputed them in its SHADE stage: the same
// expressions, so the same bits). The light record is wave-uniform and comes through the scalar cache.
//
// Registers: nothing but the accumulated colour, the distance to the light and the material tag is live across a shadow ray's
// walk besides the ray itself (the ray's origin IS the hit point, its direction IS the light direction); the shading normal and
// the incoming direction wait in the lane's LDS column.
#pragma once

#include "pt_shade.h"

// The certain-shadow test (pt_certain.h) exists in the mesh-free flat_scene kernels only. Objects compiled for another mode (-DPT_INST_MODE) keep a light's set-up as
// it was, line for line, and so does every object under -DPT_NO_CERTAIN_SHADOW: the two forms compute the same, but the compiler allocates registers differently
// for them (the chain kernel of scenes with meshes lost 1.8 % to the new form alone).
#if !defined(PT_NO_CERTAIN_SHADOW) && (!defined(PT_INST_MODE) || PT_INST_MODE == 3)
#define PT_CERTAIN_SHADOW_FORM 1
#endif

// The per-pixel candidate lists of the primary stage (pt_pixel_list.h) exist where the eye table does: the plain mesh-free flat_scene kernels. Every other mode's object
// keeps its text, and so does every object under -DPT_NO_PIXEL_LISTS (A/B: the kernels as they were, and the host fills no lists).
#if !defined(PT_NO_PIXEL_LISTS) && !defined(PT_NO_EYE_TABLE) && (!defined(PT_INST_MODE) || PT_INST_MODE == 3)
#define PT_PIXEL_LIST_FORM 1
#include "pt_pixel_list.h"
// The queue of the pixels that need the kernel (pt_pixel_list.h: PT_PL_QUEUE): where the launch has one, the instantiations that have PIXEL_LISTS deal its entries instead
// of every pixel of the launch. -DPT_NO_BACKGROUND_SKIP: the kernels as they were (A/B), and the host asks for no queue.
#if !defined(PT_NO_BACKGROUND_SKIP)
#define PT_BACKGROUND_SKIP_FORM 1
#endif
// one or two words at a wave-uniform address through the scalar cache
typedef uint32_t pt_u32x2 __attribute__((ext_vector_type(2)));
PT_HD uint32_t pt_sload1(const void* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t v;
    asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(pt_uniform_ptr(p)) : "memory");
    return v;
#else
    return *static_cast<const uint32_t*>(p);
#endif
}
PT_HD pt_u32x2 pt_sload2(const void* p) {
    pt_u32x2 v;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_load_dwordx2 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(pt_uniform_ptr(p)) : "memory");
#else
    v = *static_cast<const pt_u32x2*>(p);
#endif
    return v;
}
// The record of work item w's pixel (pt_pixel_list.h), where the launch has lists and a wavefront is one pixel: its head - entry count or PT_PL_WALK - and tail bound through
// the scalar cache; the entries are fetched one by one where they are tested (pt_pl_eval). nullptr, *head = PT_PL_WALK: no list, the walk. Shared by the plain kernel and the
// counting build of -DPT_PIXEL_LIST_STATS, so that both read the same record the same way.
PT_HD const uint32_t* pt_pl_fetch(const PtRenderArgs& a, uint32_t n_nodes, uint32_t w, uint32_t* head, uint32_t* tail) {
    *head = PT_PL_WALK; *tail = 0u;
    if (!a.eye_tab || a.k_log2 + a.c_log2 != 6u) return nullptr;
    const uint32_t* const header = (const uint32_t*)((const char*)a.eye_tab + pt_pl_header_offset(n_nodes));
    if (pt_sload1(header) == 0u) return nullptr;
    const uint32_t slot = (pt_fastdiv(w >> 6, a.div_groups) << 6) | pt_tile_order_to_slot(w & 63u);  // (pt_item_lane_fast's, from the wave-uniform part alone)
    const uint32_t* const rec = header + 16 + (size_t)slot * PT_PL_WORDS;
    const pt_u32x2 h = pt_sload2(rec);
    *head = h[0]; *tail = h[1];
    return rec;
}
// The walk's own leaf test (same function, same range through pt_cand_end_in, same eye table) on the record's entries instead of the walk: the nearest candidate, the lowest
// index on ties, whatever the order. The entries come in ascending bound: one whose bound lies strictly above every live lane's hit ends the list - neither it nor anything
// behind it, the left-out tail included, can hold a hit at or in front of those. Returns true where the tail does not settle every live lane: the item takes the walk, from
// scratch. head: not PT_PL_WALK. *tests (may be null): the leaf tests this lane ran.
PT_HD bool pt_pl_eval(const PtSceneView& sc, const uint32_t* rec, uint32_t head, uint32_t tail, const PtRay& ray, bool live, PtHit& hit, PtCounters* cnt, const double* eye_tab,
                      unsigned long long* tests) {
    bool settled = false;
    const uint32_t n = head & 255u;
    for (uint32_t i = 0; i < n && !settled; i++) {
        const uint32_t e = pt_sload1(rec + 2 + i);
        if (PT_BALLOT(live && !((double)pt_pl_entry_bound(e) > hit.t)) == 0ull) settled = true;
        else if (live) {
            pt_test_node_uniform<false, false, true>(sc, pt_pl_entry_node(e), ray, false, hit, cnt, eye_tab);
            if (tests) (*tests)++;
        }
    }
    if (settled || tail == PT_PL_INF_BITS) return false;
    return PT_BALLOT(live && !((double)pt_f32_of(tail) > hit.t)) != 0ull;
}
#endif

// doubles at a wave-uniform address through the scalar cache (N = 2 or 4)
template <int N>
PT_HD void pt_sload_f64(const double* p, double* out) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (N == 4) {
        pt_u32x8 v = pt_sload8(p);
#pragma unroll
        for (int k = 0; k < 4; k++) out[k] = pt_f64_of(v[2 * k], v[2 * k + 1]);
    } else {
        pt_u32x4 v = pt_sload4(p);
#pragma unroll
        for (int k = 0; k < 2; k++) out[k] = pt_f64_of(v[2 * k], v[2 * k + 1]);
    }
#else
    for (int k = 0; k < N; k++) out[k] = p[k];
#endif
}

// The kernel's argument block seen AGAIN through a pointer the compiler cannot trace back to the kernarg segment: what is read
// through it is fetched (scalar loads, constant cache) where it is used instead of being kept in scalar registers from the top of
// the kernel on. The straight-line kernels keep ~200 wave-uniform values alive (scene pointers, camera, item geometry); what does
// not fit the 106 scalar registers is spilled into lanes of a vector register and comes back one v_readlane each - VALU issue slots,
// 180 of them per work item before this (38 for the camera alone, at the start of every item).
PT_HD const PtRenderArgs& pt_args_again(const PtRenderArgs& a) {
#if defined(__HIP_DEVICE_COMPILE__)
    const __attribute__((address_space(4))) PtRenderArgs* ka = (const __attribute__((address_space(4))) PtRenderArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    return *(const PtRenderArgs*)ka;
#else
    return a;
#endif
}

// Kernels whose lanes need traversal stacks of their own (KDMesh trees) split the block's LDS stack area: `rows` x 64 entries for each
// wavefront's own stack, the rest for the lanes' (which continue in HBM, PtStackSpill). The wavefront's stack has no HBM part: it gets as
// many rows as the deepest walk of THIS scene can have pending (scene.stack_cap bounds that), at the lanes' expense if need be - so a deep
// device-built tree costs lane rows, not the render (PT_ERR_TRAVERSAL is left for scenes beyond stack_lds_cap x 64 entries).
PT_HD int pt_wave_rows(const PtRenderArgs& a) {
    const int cap = a.stack_lds_cap;
    int rows = cap >= 16 ? 8 : (cap >= 8 ? 3 : (cap >= 4 ? 2 : 1));
    const int need = (a.scene.stack_cap + 63) / 64;
    if (need > rows) rows = need < cap ? need : cap;
    return rows;
}

// The block's LDS stack area in the k-d tree semantics (one walk per wavefront, pt_trace_packet_kd): `lane_rows` rows (PT_BLOCK words each)
// of per-lane stack columns - only scenes with KDMesh trees have any (pt_kdmesh_hit) -, then per wavefront `wrows` rows of 64 words:
// `srows` for its stack (a word per pending split + what a mesh's triangle tree can have pending), the rest two rows per tree level for
// the lanes' saved range bounds - the deepest levels; the top ones, touched once or twice per ray, in the lanes' HBM columns.
struct PtKdLayout { int lane_rows, wrows, srows, lds_levels, path_word; };  // path_word: where in the wavefront's region the path table starts (words)
template <int MODE>
PT_HD PtKdLayout pt_kd_layout(const PtRenderArgs& a) {
    PtKdLayout l;
    const int cap = a.stack_lds_cap;
    l.srows = (a.scene.stack_cap + 63) / 64;
    l.lane_rows = 0;
    if (MODE == PT_MODE_KD && a.scene.mkd) {
        int r = cap - l.srows - 2 * a.scene.kd_levels;
        r = r < 2 ? 2 : r;
        r = r > cap - l.srows ? cap - l.srows : r;
        l.lane_rows = r < 0 ? 0 : r;
    }
    l.wrows = cap - l.lane_rows;  // >= 1
    if (l.wrows < l.srows + 2 && 3 * a.scene.kd_levels > l.srows * 64 - a.scene.stack_cap) {  // room for the path table comes first (pt_stack_lds_cap keeps cap >= srows + 2 in these semantics)
        l.wrows = cap < l.srows + 2 ? cap : l.srows + 2;
        l.lane_rows = cap - l.wrows;
    }
    // the levels that get no slot are recomputed from the path table (PtKdSav, pt_walk_kd.h): 3 words per such level, in the slack behind the wavefront's stack
    // (its rows hold srows x 64 words, the walks need scene.stack_cap of them) or, where that is too small, in two rows taken from the level slots
    int lv = (l.wrows - l.srows) / 2;
    lv = lv < 0 ? 0 : (lv > a.scene.kd_levels ? a.scene.kd_levels : lv);
    const int slack = l.srows * 64 - a.scene.stack_cap;
    if (3 * (a.scene.kd_levels - lv) <= slack && l.wrows >= l.srows) {
        l.path_word = a.scene.stack_cap;
    } else {  // (3 x 32 levels = 96 words: two rows always do)
        lv = (l.wrows - l.srows - 2) / 2;
        lv = lv < 0 ? 0 : (lv > a.scene.kd_levels ? a.scene.kd_levels : lv);
        l.path_word = (l.srows + 2 * lv) * 64;
    }
    l.lds_levels = lv;
    return l;
}

// One ray kind for the whole wavefront: `tracing` lanes carry `ray`; result in `hit` (untouched for the other lanes).
// EYE (PT_MODE_FLAT_NOMESH only): the rays are primary rays; the walk's leaf tests take the local origin from the launch's eye table (a.eye_tab, pt_test_node_uniform).
template <int MODE, bool STATS, bool EYE = false>
PT_HD void pt_trace_wave(const PtRenderArgs& a, const PtRay& ray, bool tracing, bool any, PtHit& hit, const PtStackSpill& stk, uint32_t* lds, PtCounters* cnt,
                         PtOccRef occ = PtOccRef{nullptr, 0u, 0u}) {
#ifdef PT_CYCLES  // profiles/cycles.sh: wave cycles inside the walks -> diag[0], calls -> diag[1]
    const unsigned long long cyc_t0 = __builtin_readcyclecounter();
    struct CycEnd { unsigned long long t0; PtCounters* c; __device__ ~CycEnd() { if (STATS && (threadIdx.x & 63u) == 0) { c->diag[0] += __builtin_readcyclecounter() - t0; c->diag[1]++; } } } cyc_end{cyc_t0, cnt};
#endif
#if defined(PT_ABLATE) && (PT_ABLATE == 5 || PT_ABLATE == 6)  // measurement builds only (profiles/light_slope.py): 5 = no shadow walks (nothing is ever in the way), 6 = no walks at all
    if (any || PT_ABLATE == 6) return;
#endif
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t wave = threadIdx.x >> 6;
#else
    const uint32_t wave = 0;
#endif
    // The wavefront's stack is a linear region of the block's LDS stack area: all of the wavefront's share where no lane needs a
    // stack of its own, else the part behind the lanes' rows (KDMesh trees are walked per lane, pt_kdmesh_hit).
    if (MODE == PT_MODE_FLAT_NOMESH || MODE == PT_MODE_HIER_NOMESH) {
        const int words = a.stack_lds_cap * 64;
        constexpr bool EYE_WALK = EYE && MODE == PT_MODE_FLAT_NOMESH;
        pt_trace_packet<STATS, MODE == PT_MODE_HIER_NOMESH, EYE_WALK>(a.scene, ray, tracing, any, hit, lds + (size_t)wave * words, words, a.overflow_flag, cnt, occ, EYE_WALK ? a.eye_tab : nullptr);
    } else if (MODE == PT_MODE_FLAT || MODE == PT_MODE_HIER_MESH) {
        const int words = a.stack_lds_cap * 64;
        pt_trace_packet_mesh<STATS, false, MODE == PT_MODE_HIER_MESH>(a.scene, ray, tracing, any, hit, lds + (size_t)wave * words, words, stk, a.overflow_flag, cnt);
    } else if (MODE == PT_MODE_FLAT_KDMESH || MODE == PT_MODE_HIER) {
        const int rows = pt_wave_rows(a);  // of the wavefront's stack (64 entries each); the lanes' own stacks get the rest
        PtStackSpill lane_stk = stk;
        lane_stk.cap = a.stack_lds_cap - rows;
        pt_trace_packet_mesh<STATS, true, MODE == PT_MODE_HIER>(a.scene, ray, tracing, any, hit, lds + (size_t)lane_stk.cap * PT_BLOCK + (size_t)wave * rows * 64, rows * 64, lane_stk,
                                                                a.overflow_flag, cnt);
    } else if (MODE == PT_MODE_KD_NOMESH || MODE == PT_MODE_KD || MODE == PT_MODE_KD_MESH) {  // (pt_scene_upload refuses trees of more than PT_KD_WAVE_LEVELS levels)
        const PtKdLayout kl = pt_kd_layout<MODE>(a);
        const int lane_rows = kl.lane_rows, wrows = kl.wrows, srows = kl.srows, lds_levels = kl.lds_levels;
        PtStackSpill lane_stk = stk;
        lane_stk.cap = lane_rows;
        uint32_t* wbase = lds + (size_t)lane_rows * PT_BLOCK + (size_t)wave * wrows * 64;
        PtKdSav sav;
        sav.lds = wbase + (size_t)srows * 64;
        sav.top_levels = a.scene.kd_levels - lds_levels;
        sav.path = wbase + kl.path_word;
        int stack_words = (wrows < srows ? wrows : srows) * 64;
        if (kl.path_word < stack_words) stack_words = kl.path_word;  // (the path table sits in the slack of the stack's rows: the stack ends where it begins)
        pt_trace_packet_kd<STATS, MODE == PT_MODE_KD || MODE == PT_MODE_KD_MESH, MODE == PT_MODE_KD>(a.scene, ray, tracing, any, hit, wbase, stack_words, sav, lane_stk, a.overflow_flag, cnt);
    }
}

// The first words of the wavefront's own traversal stack (free between walks): the queue through which offered rays find takers
// (pt_render_kernel, FORK). At least 64 words: the wavefront's region is stack_lds_cap x 64 words, or `rows` x 64 behind the lanes' rows.
template <int MODE>
PT_HD uint32_t* pt_fork_queue(const PtRenderArgs& a, uint32_t* lds) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t wave = threadIdx.x >> 6;
#else
    const uint32_t wave = 0;
#endif
    if (MODE == PT_MODE_FLAT_KDMESH || MODE == PT_MODE_HIER) {
        const int rows = pt_wave_rows(a);
        return lds + (size_t)(a.stack_lds_cap - rows) * PT_BLOCK + (size_t)wave * rows * 64;
    }
    if (MODE == PT_MODE_KD || MODE == PT_MODE_KD_NOMESH || MODE == PT_MODE_KD_MESH) { const PtKdLayout kl = pt_kd_layout<MODE>(a); return lds + (size_t)kl.lane_rows * PT_BLOCK + (size_t)wave * kl.wrows * 64; }  // the first row of the wavefront's region: its stack, free between walks
    return lds + (size_t)wave * a.stack_lds_cap * 64;
}

// CHAIN (round 3): scenes whose reflective materials are all OPAQUE (reflectivity > 0, no index of refraction - the mirror scene,
// glossy metal). Their recursion (material.rs:216-243, :312-316) is a chain, not a tree: every hit spawns at most ONE ray, so the
// samples of a work item still go through the same sequence of ray kinds - bounce by bounce - and the straight line only needs a
// loop over the depth: trace, shade (shadow rays as above), and where the material reflects, park {colour so far, reflectivity} in the
// lane's HBM line of that depth and go on with the reflected ray (glossy: its two draws follow the area lights' in the sampling
// contract's order, which is this loop's order). A chain that ends - background, a matte surface, depth 10 - is folded back at once,
// innermost first: value = colour_k + value * reflectivity_k, exactly the reference's `color += reflectivity * reflected_color`.
// Lanes whose chains have ended idle until the wavefront's longest chain has; no interpreter, no stage word, no frame in LDS.
template <int MODE, bool STATS, bool TEX, int WAVES, bool CHAIN = false>
__global__ void __launch_bounds__(PT_BLOCK, WAVES) pt_render_simple_kernel(PtRenderArgs a0) {
    constexpr bool HIER = MODE == PT_MODE_HIER || MODE == PT_MODE_HIER_NOMESH || MODE == PT_MODE_HIER_MESH;
    // The primary stage of the mesh-free flat_scene kernel reads the camera's eye in each node's space from the launch's eye table (PtRenderArgs::eye_tab: filled once
    // per launch, pt_eye_table_kernel) instead of transforming it in every lane for every leaf test and once more for the surface. The counting and the chain
    // instantiations keep the per-lane transform; -DPT_NO_EYE_TABLE: every instantiation does, and no table is filled (A/B).
#if defined(PT_NO_EYE_TABLE)
    constexpr bool EYE_TABLE = false;
#else
    constexpr bool EYE_TABLE = MODE == PT_MODE_FLAT_NOMESH && !CHAIN && !STATS;
#endif
    // The surface of a hit from records fetched once per wavefront and node (pt_hit_surface_uniform_flat): the mesh-free flat_scene kernel of scenes without
    // reflection or maps. The counting instantiations keep the per-lane form;
    // -DPT_NO_UNIFORM_HIT: the per-lane form everywhere (A/B).
#if defined(PT_NO_UNIFORM_HIT)
    constexpr bool UNIFORM_HIT = false;
#else
    constexpr bool UNIFORM_HIT = MODE == PT_MODE_FLAT_NOMESH && !TEX && !CHAIN && !STATS;
#endif
    extern __shared__ uint32_t pt_lds[];
    const PtRenderArgs& a = a0;
    const uint32_t lane_global = blockIdx.x * PT_BLOCK + threadIdx.x;
    const unsigned lane = threadIdx.x & 63u;
    [[maybe_unused]] const PtSceneView& sc = a.scene;  // (shadowed per item by the re-read arguments' view)
    PtStackSpill stk;
    stk.base = pt_lds + threadIdx.x;
    stk.cap = a.stack_lds_cap;
    stk.total = a.scene.stack_cap;
    stk.gbase = a.stack_spill + lane_global;
    stk.gstride = a.n_lanes;
    stk.overflow = a.overflow_flag;
    PtFrameRef fr;
    fr.lds = reinterpret_cast<double*>(pt_lds + (size_t)a.stack_lds_cap * PT_BLOCK) + threadIdx.x;
    fr.park = fr.lds;
    fr.spill = CHAIN ? a.spill + (size_t)lane_global * (PT_SPILL_DEPTHS * PT_SPILL_STRIDE) : nullptr;
    fr.n_lanes = a.n_lanes;

    PtCounters cnt;
    if (STATS) memset(&cnt, 0, sizeof cnt);
    unsigned q_next = 0, q_end = 0, q_seen = 0;  // the wavefront's private batch of items (wave-uniform), as in pt_render_kernel
    if (a.fine_queues) q_next = blockIdx.x % a.fine_queues;
#ifdef PT_TIMELINE  // profiles/timeline.sh: when wavefronts start and end, and how long the longest item takes (100 MHz ticks), as in pt_render_kernel
    const unsigned long long tl_start = wall_clock64();
    unsigned long long tl_item_max = 0, tl_first_item = 0;
#endif
#if defined(PT_BACKGROUND_SKIP_FORM)
    // Where the launch has the queue (header word 0; a launch that has it has lists), the hand-out positions run over its entries x the chunk groups of a pixel: position
    // q is group q % groups of the pixel slot queue[q / groups]. pl_deal: the items dealt (wave-uniform, read once: the list kernel has finished); 0xFFFFFFFF: no queue.
    [[maybe_unused]] uint32_t pl_deal = 0xFFFFFFFFu;
    if constexpr (EYE_TABLE) {
        if (a.eye_tab && a.k_log2 + a.c_log2 == 6u) {
            const pt_u32x2 h = pt_sload2((const char*)a.eye_tab + pt_pl_header_offset(a.scene.n_nodes));
            if (h[0] & PT_PL_QUEUE) pl_deal = h[1] * a.div_groups.d;
        }
    }
#define PT_ITEMS_DEALT ((EYE_TABLE && pl_deal != 0xFFFFFFFFu) ? pl_deal : a.n_items)
#else
#define PT_ITEMS_DEALT a.n_items
#endif

    for (;;) {
        unsigned w;
        if (a.fine_queues == 0u) {  // guided batches from one counter (very long launches, the k-d tree semantics)
            if (q_next == q_end) {
                unsigned remaining = PT_ITEMS_DEALT > q_seen ? PT_ITEMS_DEALT - q_seen : 0u;
                unsigned take = remaining / a.work_div;
                take = take > a.batch_max ? a.batch_max : (take < 1u ? 1u : take);
                unsigned base = 0;
                if (lane == 0) base = atomicAdd(a.work_counter, take);
                base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
                q_next = base; q_end = base + take; q_seen = q_end;
            }
            const unsigned q = q_next++;
            if (q >= PT_ITEMS_DEALT) break;
            w = a.item_stride == 1u ? q : (unsigned)(((unsigned long long)q * a.item_stride) % a.n_items);  // (a launch with a queue has item_stride 1: pt_plan_launch)
        } else {  // one item at a time from interleaved queues
            for (;;) {
                unsigned idx = 0;
                if (lane == 0) idx = atomicAdd(a.work_queues + q_next * PT_QUEUE_STRIDE, 1u);
                idx = (unsigned)__builtin_amdgcn_readfirstlane((int)idx);
                const unsigned long long pos = (unsigned long long)idx * a.fine_queues + q_next;
                if (pos < PT_ITEMS_DEALT) { w = (unsigned)pos; q_end = 0; break; }
                q_next = q_next + 1u == a.fine_queues ? 0u : q_next + 1u;
                if (++q_end == a.fine_queues) { w = 0xFFFFFFFFu; break; }
            }
            if (w == 0xFFFFFFFFu) break;
        }

#ifdef PT_TIMELINE
        const unsigned long long tl_item = wall_clock64();
        if (!tl_first_item) tl_first_item = tl_item;
#endif
#ifdef PT_CYCLES  // sections of an item outside the walks: diag[3] primary ray, diag[4] surface of the hit, diag[6] light + shadow ray set-up, diag[7] light term
        const unsigned long long cyc_item0 = __builtin_readcyclecounter();
        unsigned long long sec_t0 = cyc_item0;
#define PT_SEC_SKIP() sec_t0 = __builtin_readcyclecounter()
#define PT_SEC_END(k) do { if (STATS && lane == 0) cnt.diag[k] += __builtin_readcyclecounter() - sec_t0; sec_t0 = __builtin_readcyclecounter(); } while (0)
#else
#define PT_SEC_SKIP() do { } while (0)
#define PT_SEC_END(k) do { } while (0)
#endif
        // (shadows the kernel's own view of its arguments for the rest of the item. The k-d semantics of mesh-free scenes are as fast without
        // - 30.5 against 30.7 ms on big-scene, c22 / c50 -; with mesh instances they gain like the others: mirror 8.7 -> 9.6 Gray/s, macho-cows 6.7 -> 7.2, c50)
        const PtRenderArgs& a = pt_args_again(a0);
        const PtSceneView& sc = a.scene;
        // ---- the primary ray of this lane's sample (render.rs:36-41, camera.rs:48-84)
        uint32_t x, y;
        bool mine;
        PtRay ray;
        ray.o = ray.d = pt_v3(0.0, 0.0, 0.0);
#if defined(PT_PIXEL_LIST_FORM)
        // The pixel's candidate list (pt_pl_fetch). pl_head = PT_PL_WALK: no list, today's walk.
        constexpr bool PIXEL_LISTS = EYE_TABLE;
        const uint32_t* pl_rec = nullptr;
        uint32_t pl_head = PT_PL_WALK, pl_tail = 0u;
#if defined(PT_BACKGROUND_SKIP_FORM)
        // With the queue, w is still the hand-out position: its pixel slot comes from the queue - one dependent load in place of the header word's, which such a launch
        // need not read again - and gives the record's address and the item index w that everything below uses, as if every item had been dealt.
        if (PIXEL_LISTS && pl_deal != 0xFFFFFFFFu) {
            const uint32_t* const header = (const uint32_t*)((const char*)a.eye_tab + pt_pl_header_offset(sc.n_nodes));
            const uint32_t pixel = pt_fastdiv(w, a.div_groups), group = w - pixel * a.div_groups.d;
            const uint32_t slot = pt_sload1(header + 16 + (size_t)a.n_slots * PT_PL_WORDS + pixel);
            w = ((((slot >> 6) * a.div_groups.d + group) << 6) | pt_pl_slot_to_tile_order(slot & 63u));
            pl_rec = header + 16 + (size_t)slot * PT_PL_WORDS;
            const pt_u32x2 h = pt_sload2(pl_rec);
            pl_head = h[0]; pl_tail = h[1];
        } else
#endif
        if constexpr (PIXEL_LISTS) pl_rec = pt_pl_fetch(a, sc.n_nodes, w, &pl_head, &pl_tail);
        // no leaf is reached by any ray through the pixel: background for every sample, without jitter draws, camera ray or walk
        const bool pl_background = PIXEL_LISTS && pl_head == 0u && pl_tail == PT_PL_INF_BITS;
#else
        constexpr bool pl_background = false;
#endif
        {
            PtItemLane it;
            mine = pt_item_lane_fast(a, w, lane, &it, &x, &y);
            if (mine && !pl_background) {
                double jx = 0.5, jy = 0.5;
                if (a.jitter_mode == PT_JITTER_RNG) {  // render.rs:38-39: x drawn before y
                    const uint64_t key = pt_rng_key(a.seed, (uint64_t)y * a.width + x);
                    jx = pt_rng_draw(key, it.sample, 0);
                    jy = pt_rng_draw(key, it.sample, 1);
                }
                ray = pt_camera_ray(a.cam, (double)x + jx, (double)y + jy);
                if (STATS) cnt.primary++;
            }
        }
        bool live = mine;     // the lane's chain of rays goes on (without CHAIN: one round)
        uint32_t draw = 2;    // the two jitter draws came first. CHAIN: per lane (which lanes draw depends on what their rays hit) ...
        uint32_t udraw = 2;   // ... otherwise the same for every lane: kept where the compiler can see that it is wave-uniform
        for (int depth = 0; CHAIN ? __any(live) : depth == 0; depth++) {
        PtHit hit;
        hit.t = INFINITY; hit.node = PT_NO_HIT; hit.sub = 0;
        PT_SEC_END(3);
#if defined(PT_PIXEL_LIST_STATS) && defined(PT_PIXEL_LIST_FORM)
        const unsigned long long pl_na0 = cnt.n_analytic;
#endif
#if defined(PT_PIXEL_LIST_FORM)
        // the list instead of the walk (pt_pl_eval); the walk where there is no list, or where the list's tail leaves a lane open
        bool pl_walk = true;
        if constexpr (PIXEL_LISTS) {
            if (!(pl_head & PT_PL_WALK)) pl_walk = pl_background ? false : pt_pl_eval(sc, pl_rec, pl_head, pl_tail, ray, live, hit, &cnt, a.eye_tab, nullptr);
        }
        if (pl_walk)
#endif
        pt_trace_wave<MODE, STATS, EYE_TABLE>(a, ray, live, false, hit, stk, pt_lds, &cnt);  // (EYE_TABLE is never CHAIN: this is the depth-0 walk, the only one)
#if defined(PT_PIXEL_LIST_STATS) && defined(PT_PIXEL_LIST_FORM)
        // -DPT_PIXEL_LIST_STATS (profiles/pixel_list_stats.py): the counting build evaluates the pixel's list BESIDE its unchanged walk - the plain build's procedure on a
        // hit record of its own - and counts, in 21-bit fields (fewer than 2,097,152 items: the script checks): diag[0] items with a record | of them background (empty
        // list, infinite tail) | marked "take the walk"; diag[1] items whose list was cut at the cap (finite tail) | items that would fall back to the walk | items in
        // which some lane's list result differs from the walk's (must be 0); diag[2] leaf tests by list and diag[3] by the primary walk, per lane; diag[4..7] the
        // histogram of list lengths, three bins a word: 0 .. 8, 9-10, 11-13, 14.
        // (PIXEL_LISTS is EYE_TABLE, false in a counting instantiation: this is the counting twin of the instantiations that have it - mesh-free flat_scene, no chain)
        if constexpr (STATS && MODE == PT_MODE_FLAT_NOMESH && !CHAIN) {
            {
                uint32_t head0, tail;
                const uint32_t* const rec = pt_pl_fetch(a, sc.n_nodes, w, &head0, &tail);
                if (rec) {
                    const uint32_t n = head0 & 255u;
                    const bool marked = (head0 & PT_PL_WALK) != 0u;
                    PtHit h2;
                    h2.t = INFINITY; h2.node = PT_NO_HIT; h2.sub = 0;
                    const bool walk2 = marked || pt_pl_eval(sc, rec, head0, tail, ray, live, h2, &cnt, a.eye_tab, &cnt.diag[2]);
                    const bool differs = live && !walk2 && (h2.node != hit.node || (h2.node != PT_NO_HIT && (h2.sub != hit.sub || h2.t != hit.t)));
                    const bool any_differs = PT_BALLOT(differs) != 0ull;
                    cnt.diag[3] += cnt.n_analytic - pl_na0;
                    if (lane == 0) {
                        cnt.diag[0] += 1ull | ((!marked && n == 0u && tail == PT_PL_INF_BITS) ? 1ull << 21 : 0ull) | (marked ? 1ull << 42 : 0ull);
                        cnt.diag[1] += ((!marked && tail != PT_PL_INF_BITS) ? 1ull : 0ull) | ((walk2 && !marked) ? 1ull << 21 : 0ull) | (any_differs ? 1ull << 42 : 0ull);
                        const uint32_t bin = marked ? 11u : (n <= 8u ? n : (n <= 10u ? 9u : (n <= 13u ? 10u : 11u)));
                        if (!marked) cnt.diag[4 + bin / 3u] += 1ull << (21u * (bin % 3u));
                    }
                }
            }
        }
#endif
        PT_SEC_SKIP();

        // ---- ray.rs:139-148: the background where nothing was hit, else Material::hit_color (material.rs:91-243)
        const bool shaded = live && hit.node != PT_NO_HIT;
        bool ended = live && !shaded;  // this lane's chain ends in this round: `value` is set, the parked colours get folded in
        PtVec3 value = pt_v3(0.0, 0.0, 0.0);  // (not kept in registers across the rounds: a finished chain's colour goes to the lane's LDS column at once)
        if (ended) value = pt_background(a, x, y);
        if (__any(shaded)) {
            uint32_t mat = 0, ftag = 0;
            PtRay sray;  // o = the hit point for every light; d = the direction to the light being tested
            sray.o = sray.d = pt_v3(0.0, 0.0, 0.0);
            PtVec3 color = pt_v3(0.0, 0.0, 0.0);
            PtVec3 N = pt_v3(0.0, 0.0, 0.0);
            bool surfaced = false;  // this lane's surface came from the wave-uniform form
            if (UNIFORM_HIT) {
                // One pass per DISTINCT node among the shaded lanes' hits (one pass unless the pixel's samples straddle a silhouette): the node of the first lane
                // still pending, the lanes that share it, its records as scalar operands (pt_hit_surface_uniform_flat). Triangles stay pending for the per-lane form.
                unsigned long long pending = PT_BALLOT(shaded);
                [[maybe_unused]] unsigned passes = 0;
                while (pending) {
                    const uint32_t node = (uint32_t)__builtin_amdgcn_readlane((int)hit.node, __builtin_ctzll(pending));
                    const bool here = shaded && hit.node == node;
                    pending &= ~PT_BALLOT(here);
                    const pt_u32x4 info = pt_sload4(sc.info + 4 * (size_t)node);
                    if (info[0] == PT_TRIANGLE || info[0] == PT_MESH || info[0] == PT_KDMESH) continue;
                    passes++;
                    if (here) {
                        pt_hit_surface_uniform_flat<EYE_TABLE>(sc, node, info[0], ray, hit, &sray.o, &N, a.eye_tab);
                        mat = info[3];
                        surfaced = true;
                    }
                }
            }
            if (shaded) {
                if (STATS) cnt.hits++;
                if (!surfaced) {
                    if (EYE_TABLE && UNIFORM_HIT) {
                        // what the loop above left: stand-alone triangles. Their local origin is transformed per lane from the eye re-read from the argument block (a scalar
                        // operand) - with the table gathered per lane here as well the headline instantiation spills 33 registers instead of 25
                        PtRay pr;
                        pr.o = pt_v3(a.cam.eye[0], a.cam.eye[1], a.cam.eye[2]); pr.d = ray.d;
                        pt_hit_surface<TEX, HIER>(sc, pr, hit, &sray.o, &N, &mat, &ftag);
                    } else {
                        pt_hit_surface<TEX, HIER, false, false, EYE_TABLE>(sc, ray, hit, &sray.o, &N, &mat, &ftag, a.eye_tab);
                    }
                }
                fr.set_l3(PT_L_N, N);
                fr.set_l3(PT_L_D, ray.d);
                const double* m = sc.materials + 10 * (size_t)mat;
                PtVec3 kd = pt_v3(m[0], m[1], m[2]);
                if (TEX && (ftag & PT_FS_TEXEL)) kd = pt_v3(sc.srgb_lut[ftag & 255u], sc.srgb_lut[(ftag >> 8) & 255u], sc.srgb_lut[(ftag >> 16) & 255u]);
                color = pt_v3(sc.ambient[0], sc.ambient[1], sc.ambient[2]) * kd;  // material.rs:148
                // the colour so far and the distance to the light wait in the lane's LDS column (slots of P and the tag, unused here) while the shadow ray is walked: eight registers the walks need more
                fr.set_l3(PT_L_P, color);
            }
            PT_SEC_END(4);
            for (uint32_t li = 0; li < sc.n_lights; li++) {  // material.rs:149-210, one light after the other
                const double* light = sc.lights + 15 * (size_t)li;
                double lp[4], la[2], lb[4];  // position (+ colour.x), area_a.xy, area_a.z + area_b
                pt_sload_f64<4>(light, lp);
                pt_sload_f64<2>(light + 9, la);
                pt_sload_f64<4>(light + 11, lb);
                PtVec3 lpos = pt_v3(lp[0], lp[1], lp[2]);
                const PtVec3 aa = pt_v3(la[0], la[1], lb[0]), ab = pt_v3(lb[1], lb[2], lb[3]);
                const bool area = !((aa.x == 0.0 && aa.y == 0.0 && aa.z == 0.0) || (ab.x == 0.0 && ab.y == 0.0 && ab.z == 0.0));  // light.rs:51-53 (wave-uniform)
#if !defined(PT_CERTAIN_SHADOW_FORM)  // a light's set-up as it was before the certain-shadow test, line for line
                double light_dist = 0.0;
                if (shaded) {
                    if (area) {  // light.rs:62-70, :87-90
                        PtItemLane it;
                        uint32_t x2, y2;
                        pt_item_lane_fast(a, w, lane, &it, &x2, &y2);
                        const uint64_t key = pt_rng_key(a.seed, (uint64_t)y * a.width + x);
                        const uint32_t d0 = CHAIN ? draw : udraw;
                        double a_coord = 2.0 * pt_rng_draw(key, it.sample, d0) - 1.0;
                        double b_coord = 2.0 * pt_rng_draw(key, it.sample, d0 + 1) - 1.0;
                        lpos = lpos + (aa * a_coord + ab * b_coord);
                        if (CHAIN) draw += 2;
                    }
                    PtVec3 hit_to_light = lpos - sray.o;
                    light_dist = pt_length(hit_to_light);
                    sray.d = hit_to_light / light_dist;
                    fr.l(PT_L_TAG) = light_dist;
                    if (STATS) cnt.shadow++;
                }
                if (area) udraw += 2;
                PtHit sh;
                sh.t = INFINITY; sh.node = PT_NO_HIT; sh.sub = 0;
                PT_SEC_END(6);
                // the occluder table's entry of this item's tile for this light (pt_trace_packet): mesh-free scenes, primary hits only
                PtOccRef occ{nullptr, 0u, li};
#ifdef PT_OCCLUDER_STATS
                constexpr bool OCC = !CHAIN && (MODE == PT_MODE_FLAT_NOMESH || MODE == PT_MODE_HIER_NOMESH);
#else
                constexpr bool OCC = !STATS && !CHAIN && (MODE == PT_MODE_FLAT_NOMESH || MODE == PT_MODE_HIER_NOMESH);
#endif
                if (OCC && a.occluders) {
                    const uint32_t tile_local = pt_fastdiv(w >> (a.k_log2 + a.c_log2), a.div_groups);
                    occ.entry = a.occluders + (size_t)tile_local * sc.n_lights + li;
                    occ.back = tile_local >= a.occ_row ? a.occ_row * sc.n_lights : 0u;
                }
#else
                double light_dist = 0.0;
                if (shaded && area) {  // light.rs:62-70, :87-90
                    PtItemLane it;
                    uint32_t x2, y2;
                    pt_item_lane_fast(a, w, lane, &it, &x2, &y2);
                    const uint64_t key = pt_rng_key(a.seed, (uint64_t)y * a.width + x);
                    const uint32_t d0 = CHAIN ? draw : udraw;
                    double a_coord = 2.0 * pt_rng_draw(key, it.sample, d0) - 1.0;
                    double b_coord = 2.0 * pt_rng_draw(key, it.sample, d0 + 1) - 1.0;
                    lpos = lpos + (aa * a_coord + ab * b_coord);
                    if (CHAIN) draw += 2;
                }
                if (area) udraw += 2;
#ifdef PT_OCCLUDER_STATS
                constexpr bool OCC = !CHAIN && (MODE == PT_MODE_FLAT_NOMESH || MODE == PT_MODE_HIER_NOMESH);
#else
                constexpr bool OCC = !STATS && !CHAIN && (MODE == PT_MODE_FLAT_NOMESH || MODE == PT_MODE_HIER_NOMESH);
#endif
                // A light the launch found enclosed in a node's certain ball (pt_dark_light, pt_certain.h 4.-8.; its record lies in front of the occluder table) is dark from
                // every origin the lane guard lets through: where every shaded lane passes, the light is skipped before anything is read for it - no occluder entry, no ball,
                // no direction, no probe, no walk. Otherwise today's code for that light, for all lanes. -DPT_NO_DARK_LIGHTS: the code as it was, and no records. The counting
                // build of -DPT_OCCLUDER_STATS=2 evaluates the guard and hands the outcome to pt_trace_packet's counts, nothing else.
                [[maybe_unused]] bool dark = false;
#if !defined(PT_NO_DARK_LIGHTS)
                if (OCC && MODE == PT_MODE_FLAT_NOMESH && a.occluders) {
                    const pt_u32x4 dk = pt_sload4(a.occluders - PT_DARK_WORDS * (size_t)(sc.n_lights - li));
                    if (dk[3] != 0u) {
                        float drec[4];
#pragma unroll
                        for (int k = 0; k < 4; k++) drec[k] = __builtin_bit_cast(float, (uint32_t)dk[k]);
                        const bool g = shaded & pt_dark_lane(drec, pt_f32_here(sray.o.x), pt_f32_here(sray.o.y), pt_f32_here(sray.o.z));
                        const unsigned long long want = PT_BALLOT(shaded);
                        dark = want != 0ull && PT_BALLOT(g) == want;  // (a wavefront without a shaded lane takes today's path)
                        if (!STATS && dark) { PT_SEC_END(6); continue; }
                    }
                }
#endif
                // the occluder table's entry of this item's tile for this light (pt_trace_packet): mesh-free scenes, primary hits only
                PtOccRef occ{nullptr, 0u, li};
                if (OCC && a.occluders) {
                    const uint32_t tile_local = pt_fastdiv(w >> (a.k_log2 + a.c_log2), a.div_groups);
                    occ.entry = a.occluders + (size_t)tile_local * sc.n_lights + li;
                    occ.back = tile_local >= a.occ_row ? a.occ_row * sc.n_lights : 0u;
                }
                // Where the candidate's inscribed ball (the launch's table, pt_certain.h) settles every shaded lane - the exact ray certainly ends in that node - the
                // light contributes nothing to this item: no direction, no length, no probe, no walk. The entry is written as the probe would have written it.
                // Flat_scene semantics only: the hierarchical one has no composed forward record resident to place the balls with. -DPT_NO_CERTAIN_SHADOW: the
                // code as it was, and no table. The counting build of -DPT_OCCLUDER_STATS=2 evaluates the test and hands the outcome to pt_trace_packet's counts,
                // nothing else.
                constexpr bool CERTAIN = OCC && MODE == PT_MODE_FLAT_NOMESH;
                [[maybe_unused]] PtOccHint hint{0u, 0u, 0u, (STATS && dark) ? 4u : 0u};
                if (CERTAIN && occ.entry) {  // (a launch of this mode that has an occluder table has the certain-shadow table: pt_plan_launch)
                    const float* const certain_tab = (const float*)(a.eye_tab + 12 * (size_t)sc.n_nodes);
                    const uint32_t* const entry = (const uint32_t*)pt_uniform_ptr(occ.entry);
                    hint.own = PT_UNIFORM_U32(entry[0]);
                    hint.up = occ.back ? PT_UNIFORM_U32(entry[-(long)occ.back]) : 0u;
                    hint.loaded = 1u;
                    const uint32_t cand = hint.own ? hint.own : hint.up;
                    if (cand != 0u) {
                        const pt_u32x4 rec = pt_sload4(certain_tab + 4 * (size_t)(cand - 1u));
                        float ball[4];
#pragma unroll
                        for (int k = 0; k < 4; k++) ball[k] = __builtin_bit_cast(float, (uint32_t)rec[k]);
                        if (ball[3] > 0.0f) {
                            const float pf[3] = {pt_f32_here(sray.o.x), pt_f32_here(sray.o.y), pt_f32_here(sray.o.z)};
                            const float lx = (float)lpos.x, ly = (float)lpos.y, lz = (float)lpos.z;
                            const bool c1 = shaded && pt_certain_lane(ball, pf[0], pf[1], pf[2], lx, ly, lz);
                            const unsigned long long want = PT_BALLOT(shaded), got = PT_BALLOT(c1);
                            bool settled = want != 0ull && got == want;  // (a wavefront without a shaded lane writes no entry, like the probe)
                            if (settled) {
                                hint.certain |= 3u;
                                if (!STATS && hint.own != cand && lane == (unsigned)(__ffsll((long long)__ballot(1)) - 1)) occ.entry[0] = cand;
                            }
                            if (!STATS && settled) { PT_SEC_END(6); continue; }  // (PT_CYCLES builds count STATS instantiations only, which never get here)
                        }
                    }
                }
                if (shaded) {
                    PtVec3 hit_to_light = lpos - sray.o;
                    light_dist = pt_length(hit_to_light);
                    sray.d = hit_to_light / light_dist;
                    fr.l(PT_L_TAG) = light_dist;
                    if (STATS) cnt.shadow++;
                }
                PtHit sh;
                sh.t = INFINITY; sh.node = PT_NO_HIT; sh.sub = 0;
                PT_SEC_END(6);
#endif
#if defined(PT_CERTAIN_SHADOW_FORM) && !defined(PT_CYCLES) && !defined(PT_ABLATE)
                if (CERTAIN && occ.entry) {  // the table's test with the entries read above (what pt_trace_wave does for this mode, and pt_trace_packet behind it)
                    const int words = a.stack_lds_cap * 64;
                    pt_trace_packet_occ<STATS, false>(sc, sray, shaded, sh, pt_lds + (size_t)(threadIdx.x >> 6) * words, words, a.overflow_flag, &cnt, occ, hint);
                } else
#endif
                pt_trace_wave<MODE, STATS>(a, sray, shaded, true, sh, stk, pt_lds, &cnt, occ);  // material.rs:174-179 only asks whether anything is in the way
                PT_SEC_SKIP();
                if (shaded && sh.node == PT_NO_HIT) {
                    double lc[2], lf[4];  // colour.xy, colour.z + falloff
                    pt_sload_f64<2>(light + 3, lc);
                    pt_sload_f64<4>(light + 5, lf);
                    const double* m = sc.materials + 10 * (size_t)mat;
                    PtVec3 kd = pt_v3(m[0], m[1], m[2]), ks = pt_v3(m[3], m[4], m[5]);
                    if (TEX && (ftag & PT_FS_TEXEL)) kd = pt_v3(sc.srgb_lut[ftag & 255u], sc.srgb_lut[(ftag >> 8) & 255u], sc.srgb_lut[(ftag >> 16) & 255u]);
                    fr.set_l3(PT_L_P, fr.l3(PT_L_P) + pt_light_term(pt_v3(lc[0], lc[1], lf[0]), pt_v3(lf[1], lf[2], lf[3]), sray.d, fr.l(PT_L_TAG), fr.l3(PT_L_N), fr.l3(PT_L_D), kd, ks, m[6]));
                }
                PT_SEC_END(7);
            }
            if (shaded) {
                color = fr.l3(PT_L_P);
                const double* m = sc.materials + 10 * (size_t)mat;
                const double reflectivity = m[7], glossy = m[8];
                if (!CHAIN || !(reflectivity > 0.0)) {  // material.rs:216: nothing is reflected
                    value = color; ended = true;
                } else if (depth + 1 > PT_MAX_DEPTH) {  // the reflected ray would be a depth-11 ray: its colour is the background (material.rs:102-104), not traced
                    if (STATS) cnt.depth11_skipped++;
                    value = color + pt_background(a, x, y) * reflectivity;  // material.rs:312-316
                    ended = true;
                } else {
                    const PtVec3 ray_dir = fr.l3(PT_L_D), N = fr.l3(PT_L_N);
                    PtVec3 reflect_dir = ray_dir - (N * 2.0) * pt_dot(ray_dir, N);  // material.rs:218
                    if (glossy > 0.0) {  // material.rs:221-239 (not renormalised: quirk Q5)
                        PtVec3 off = (fabs(reflect_dir.x) < PT_EPSILON && fabs(reflect_dir.y) < PT_EPSILON) ? reflect_dir + pt_v3(0.0, 0.1, 0.0) : reflect_dir + pt_v3(0.0, 0.0, 0.1);
                        PtVec3 u_basis = pt_cross(reflect_dir, off);
                        PtVec3 v_basis = pt_cross(reflect_dir, u_basis);
                        PtItemLane it;
                        uint32_t x2, y2;
                        pt_item_lane_fast(a, w, lane, &it, &x2, &y2);
                        const uint64_t key = pt_rng_key(a.seed, (uint64_t)y * a.width + x);
                        double u_coord = -glossy / 2.0 + pt_rng_draw(key, it.sample, draw) * glossy;
                        double v_coord = -glossy / 2.0 + pt_rng_draw(key, it.sample, draw + 1) * glossy;
                        draw += 2;
                        reflect_dir = reflect_dir + (u_basis * u_coord + v_basis * v_coord);
                    }
                    double* line = fr.spill + (size_t)depth * PT_SPILL_STRIDE;  // parked until the chain ends: colour so far, reflectivity
                    line[0] = color.x; line[1] = color.y; line[2] = color.z; line[3] = reflectivity;
                    ray.o = sray.o; ray.d = reflect_dir;
                    if (STATS) cnt.reflect++;
                }
            }
        }
        if (CHAIN && ended) {  // fold the parked colours back, innermost first (material.rs:312-316 at every level)
            for (int k = depth - 1; k >= 0; k--) {
                const double* line = fr.spill + (size_t)k * PT_SPILL_STRIDE;
                value = pt_v3(line[0], line[1], line[2]) + value * line[3];
            }
        }
        if (ended) { fr.set_l3(PT_L_VALUE, value); live = false; }
        }

        // render.rs:36-43 under the summation contract: the chunk's samples in ascending order, added by the lane of the chunk's
        // first sample from its neighbours' LDS columns (same wavefront: program order suffices).
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        {
            PtItemLane it;
            uint32_t x2, y2;
            const bool mine2 = pt_item_lane_fast(a, w, lane, &it, &x2, &y2);
            if (mine2 && it.first) {
                PtVec3 sum = fr.l3(PT_L_VALUE);
                for (uint32_t k = 1; k < it.count && k < PT_SAMPLE_CHUNK; k++) {  // (bounded by a constant as well: a corrupted count must not spin - profiles/r04/notes.md)
                    const double* o = fr.lds + k;
                    sum = sum + pt_v3(o[(PT_L_VALUE + 0) * PT_FRAME_STRIDE], o[(PT_L_VALUE + 1) * PT_FRAME_STRIDE], o[(PT_L_VALUE + 2) * PT_FRAME_STRIDE]);
                }
                // pixel-major: where a wavefront is one pixel (SAMPLES = 64) the eight chunk-first lanes' 24-byte stores fill one 192-byte run instead of eight
                // lines 1,536 bytes apart (round 3: 0.97 GB HBM-side per big-scene frame for 0.45 GB of payload, the write granularity's doing)
                double* o = a.accum + 3 * ((size_t)it.slot * a.n_chunks + it.chunk);
                o[0] = sum.x; o[1] = sum.y; o[2] = sum.z;
            }
        }
        __builtin_amdgcn_wave_barrier();
#ifdef PT_CYCLES  // the whole item -> diag[2] (the part outside the walks = diag[2] - diag[0])
        if (STATS && lane == 0) cnt.diag[2] += __builtin_readcyclecounter() - cyc_item0;
#endif
#ifdef PT_TIMELINE
        { const unsigned long long d = wall_clock64() - tl_item; if (d > tl_item_max) tl_item_max = d; }
#endif
    }
#ifdef PT_TIMELINE
    if (STATS && lane == 0) {
        const unsigned long long tl_end = wall_clock64();
        cnt.diag[0] = tl_end - tl_start; cnt.diag[1] = 1;                       // summed: wavefront lifetimes, wavefronts
        atomicMax(&a0.counters->diag[2], tl_item_max);                            // longest item
        atomicMax(&a0.counters->diag[4], ~tl_start);                              // ~(earliest start)
        atomicMax(&a0.counters->diag[5], tl_end);                                 // latest end
        cnt.diag[3] = tl_first_item ? tl_first_item - tl_start : 0;               // summed: start -> first item in hand
        atomicMax(&a0.counters->diag[6], ~tl_end);                                // ~(earliest end): the tail is latest end - earliest end
        cnt.diag[2] = cnt.diag[4] = cnt.diag[5] = cnt.diag[6] = 0;
    }
#endif
    if (STATS) pt_flush_counters(a.counters, cnt);
}
#undef PT_ITEMS_DEALT
