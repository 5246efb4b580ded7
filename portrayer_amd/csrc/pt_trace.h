// Nearest-hit / any-hit traversal: replaces `scene.root.ray_cast(ray, &mut t_range)`.
//
// FLAT mode reproduces the reference's flat_scene semantics (ray.rs:87-99 fold over
// Vec<FlatSceneNode>, flat_scene.rs:71-99): every candidate is tested in ITS OWN model space over
// [EPSILON, t_best) and the nearest wins, the lowest flat index winning exact ties. That result
// does not depend on the order candidates are visited in, so the kernels walk a bounding-volume
// tree built by pt_scene_upload instead of scanning all nodes, and break exact ties by index.
//
// KD mode reproduces the reference's `kdtree` feature bit for bit (kdtree/node.rs:66-203): the
// reference's own tree (built on the host like kdtree/leaf.rs:89-231), front-to-back with the
// range clipped at every straddled plane, because Cone/Cylinder results depend on the clipped
// range start (quirk Q1, cone.rs:64-76).
//
// The traversal stack lives in LDS: one column of 32-bit words per lane (word i of lane l at
// base[i * stride + l]) so that a wave's pushes and pops hit 64 different banks.
//
// The walks themselves are in three files included below, in this order: pt_walk_lane.h (stacks, the f32 slab tests, the walks every lane makes
// by itself), pt_walk_wave.h (ONE walk per wavefront in the flat_scene and hierarchical semantics) and pt_walk_kd.h (the same in the k-d semantics).
#pragma once

#include "pt_prims.h"
#include "pt_certain.h"
#include "pt_scene_view.h"

#define PT_NO_HIT 0xFFFFFFFFu
#define PT_WALK_POPS_MAX (1u << 27)  // watchdog of the wave-uniform walks: more pending subtrees than the largest tree (2^26 nodes) has
#define PT_BLOCK 256              // threads per block of every traversal kernel = stride of the per-lane LDS columns
#define PT_FRAME_STRIDE PT_BLOCK

// -DPT_DIAG (profiles/diag.sh): one count per WAVEFRONT pass through a place, next to the per-lane counts the
// STATS build keeps anyway; their ratio is the lane occupancy of that place.
#ifdef PT_DIAG
#define PT_WAVE_COUNT(k) do { if (STATS && (int)__lane_id() == __ffsll((long long)__ballot(1)) - 1) cnt->diag[k]++; } while (0)
#define PT_LANE_COUNT(k) do { if (STATS) cnt->diag[k]++; } while (0)
#else
#define PT_WAVE_COUNT(k) do { } while (0)
#define PT_LANE_COUNT(k) do { } while (0)
#endif
// -DPT_CYCLES (profiles/cycles.sh): shader cycles a wavefront spends in a section, summed over wavefronts into diag[k]
// (only lane 0 of a wave adds; s_memtime itself costs ~10 % of wave cycles, so read the split, not the totals)
#ifdef PT_CYCLES
#define PT_CYC_BEGIN() const unsigned long long pt_cyc0_ = __builtin_readcyclecounter()
#define PT_CYC_END(k) do { if (STATS && (__lane_id() == 0 || __ffsll((long long)__ballot(1)) - 1 == (int)__lane_id())) cnt->diag[k] += __builtin_readcyclecounter() - pt_cyc0_; } while (0)
#else
#define PT_CYC_BEGIN() do { } while (0)
#define PT_CYC_END(k) do { } while (0)
#endif

#include "pt_walk_lane.h"
#include "pt_walk_wave.h"
#include "pt_walk_kd.h"

// Traversal of one ray in the semantics of `MODE` (PT_MODE_*).
template <int MODE, bool STATS, class Stack>
PT_HD void pt_trace(const PtSceneView& sc, const PtRay& ray, bool any, PtHit& hit, const Stack& stk, PtCounters* cnt) {
    if (MODE == PT_MODE_KD || MODE == PT_MODE_KD_MESH) pt_trace_kd<STATS, true>(sc, ray, any, hit, stk, cnt);
    else if (MODE == PT_MODE_KD_NOMESH) pt_trace_kd<STATS, false>(sc, ray, any, hit, stk, cnt);
    else if (MODE == PT_MODE_FLAT_NOMESH) pt_trace_flat_simple<STATS>(sc, ray, any, hit, stk, cnt);
    else if (MODE == PT_MODE_FLAT_KDMESH) pt_trace_flat<STATS, true, true>(sc, ray, any, hit, stk, cnt);
    else if (MODE == PT_MODE_HIER) pt_trace_flat<STATS, true, true, true>(sc, ray, any, hit, stk, cnt);
    else if (MODE == PT_MODE_HIER_NOMESH) pt_trace_flat<STATS, false, false, true>(sc, ray, any, hit, stk, cnt);
    else if (MODE == PT_MODE_HIER_MESH) pt_trace_flat<STATS, true, false, true>(sc, ray, any, hit, stk, cnt);
    else pt_trace_flat<STATS, true, false>(sc, ray, any, hit, stk, cnt);
}
