// One traversal mode's instantiation of pt_segments_kernel (pt_segments.h) and its launcher. Compiled once per mode, -DPT_INST_MODE=1..9
// (Makefile: pt_segments_m<mode>.o), beside the ray-query pass's objects and through the same check / repair of the assembly.
//
// The one translation unit in which the wavefront walks of the flat_scene and hierarchical semantics do NOT start at infinity (pt_walk_wave.h, PT_WALK_ENTRY_T):
// a lane enters with best.t = its t_max, and the slab tests prune with that bound's f32 image from the first box on; a KDMesh instance's own tree is walked over
// the unbounded range and its hit filtered (PT_WALK_KDMESH_HIT), and a Mesh instance's box is tested over the unbounded range (PT_WALK_MESH_BOX_END), both while
// the lane has found nothing: the two tests whose outcome for a hit just inside the bound depends on more than the exact comparison t < t_max.
#define PT_WALK_ENTRY_T(best) (best).t
#define PT_WALK_ENTRY_TM(best) pt_tmax32((best).t)
#define PT_WALK_KDMESH_HIT(STATS, HIER, sc, mi, lr, best, node, lane_stk, t, tri, cnt) pt_kdmesh_hit_filtered<STATS, HIER>(sc, mi, lr, best, node, lane_stk, t, tri, cnt)
#define PT_WALK_MESH_BOX_END(HIER, sc, best, node) ((best).node == PT_NO_HIT ? (double)INFINITY : pt_cand_end_in<HIER>(sc, best, node, 0))
#include "pt_segments.h"

#ifndef PT_INST_MODE
#error "compile with -DPT_INST_MODE=<PT_MODE_*>"
#endif
#define PT_INST_CAT2(a, b) a##b
#define PT_INST_CAT(a, b) PT_INST_CAT2(a, b)

hipError_t PT_INST_CAT(pt_segments_launch_mode_, PT_INST_MODE)(const PtSegmentsArgs& a, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    return pt_segments_launch<PT_INST_MODE>(a, n_cu, stream, grid, launch);
}
