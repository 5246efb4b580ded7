// One traversal mode's instantiations of pt_render_kernel (counting / plain, textured / untextured,
// the variants listed in pt_render_kernel.h) and their launcher. Compiled once per mode: -DPT_INST_MODE=1..9 (Makefile).
// The texture routine (pt_apply_maps) is out of line so that untextured hits keep their register budget - except in the flat_scene
// kernels of scenes with KDMesh trees, where inlining it measured +10 % (transmission-refraction 11.5 -> 12.6 Gray/s; the same scene
// in the hierarchical semantics loses 7 % inlined: profiles/r03/notes.md section 4). In that instantiation the interpreter also applies
// the maps BEFORE it enters its state machine (PT_MAPS_BEFORE, round 4: 12.9 -> 13.6 Gray/s, 148 -> 95 GB HBM-side per frame; the
// hierarchical instantiation loses 4 % that way and keeps the call inside pt_hit_surface: profiles/r04/notes.md section 6).
#if defined(PT_INST_MODE) && PT_INST_MODE == 4
#define PT_MAPS_INLINE
#define PT_MAPS_BEFORE
#endif
// The mesh-free flat_scene kernels (mode 3: water-glass): the interpreter's map stage in front of the state machine too, with the routine's body in place THERE only
// (16.0 -> 17.3 Gray/s, c41 / c44; inline everywhere in that mode: 16.2; the hierarchical mesh-free mode 6 loses either way and keeps the call inside pt_hit_surface).
#if defined(PT_INST_MODE) && PT_INST_MODE == 3
#define PT_MAPS_BEFORE
#define PT_LANE_MAPS_INLINE
#endif
// The hierarchical kernels of scenes with KDMesh trees (mode 5, PT_MODE_HIER) keep the walks' ray constants with f64 products (pt_walk_lane.h: pt_raypk_axis_f64). With the f32 body
// this toolchain's register allocator leaves a spill store of a register pair nothing has written in pt_render_kernel<5, true, true, 3>, which LLVM's machine
// verifier refuses (`make verify-mi`: "Using an undefined physical register"); every other mode's object passes it with the f32 body.
#if defined(PT_INST_MODE) && PT_INST_MODE == 5
#define PT_RAYPK_F64
#endif
#include "pt_render_kernel.h"
#include "pt_render_inst.h"

#ifndef PT_INST_MODE
#error "compile with -DPT_INST_MODE=<PT_MODE_*>"
#endif
#define PT_INST_CAT2(a, b) a##b
#define PT_INST_CAT(a, b) PT_INST_CAT2(a, b)

hipError_t PT_INST_CAT(pt_launch_mode_, PT_INST_MODE)(const PtRenderArgs& a, int variant, bool stats, bool tex, int n_cu, hipStream_t stream,
                                                      uint32_t* grid, bool launch) {
    return pt_dispatch_variant<PT_INST_MODE>(a, variant, stats, tex, n_cu, stream, grid, launch);
}
