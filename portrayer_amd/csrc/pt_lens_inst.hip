// One traversal mode's instantiations of pt_lens_kernel - the film's sampling kernel behind a lens (pt_film_add_lens, include/portrayer_hip.h) -
// and their launcher. Compiled once per mode, -DPT_INST_MODE=1..9 (Makefile: pt_lens_m<mode>.o), beside the film's objects and through the same check / repair
// of the assembly.
//
// Every pixel of a slice gets its NEXT samples exactly as pt_film_kernel (pt_film.h) gives them - the same work item (one wavefront = 64 / K pixel slots of an
// 8x8 tile x K lanes per pixel, pt_film_item_slot), the same staging writes for pt_film_fold_kernel behind it: the film's begin and finish on the PtFilmArgs at
// the start of the block - and only the primary ray of a sample differs: it is the lens contract's (pt_lens.h), made in registers where the sample starts. No ray
// is ever in memory. The lens' four fields are read through the kernarg segment inside the source policy (PtLensSource, pt_lens_inst.h): scalar loads, the
// model's branch is wave-uniform.
#include "pt_film.h"
#include "pt_lens_inst.h"

#ifndef PT_INST_MODE
#error "compile with -DPT_INST_MODE=<PT_MODE_*>"
#endif
#define PT_INST_CAT2(a, b) a##b
#define PT_INST_CAT(a, b) PT_INST_CAT2(a, b)

template <int MODE, bool TEX, int PARK>
__global__ void pt_lens_kernel(PtLensArgs a0);

// The pass's policy for pt_shade_frame: the film's, with the lens as the source
struct PtLensPass : PtShadeItems {
    using Args = PtLensArgs;
    using Source = PtLensSource;
    using Item = PtFilmPass::Item;
    static PT_HD const PtRenderArgs& render(const PtLensArgs& a0) { return a0.f.r; }
    template <int MODE, bool TEX, int PARK>
    static constexpr auto kernel() { return &pt_lens_kernel<MODE, TEX, PARK>; }

    static __device__ __forceinline__ void begin(const PtLensArgs& a0, const PtRenderArgs& a, unsigned w, unsigned lane, Item& it, PtLane& L, const PtFrameRef& fr) {
        PtFilmPass::begin(a0.f, a, w, lane, it, L, fr);
    }
    static __device__ __forceinline__ void source(const PtLensArgs& aa, PtLensSource& src) { src.lens = &aa.lens; }  // (aa: the block as the kernarg segment shows it)
    static __device__ __forceinline__ void finish(const PtLensArgs& a0, unsigned w, unsigned lane, const Item& it, const PtLane& L, const PtFrameRef& fr) {
        PtFilmPass::finish(a0.f, w, lane, it, L, fr);  // (f is FIRST: the film's block seen again is this block's start)
    }
};

template <int MODE, bool TEX, int PARK>
__global__ void __launch_bounds__(PT_BLOCK, pt_lens_waves(MODE)) pt_lens_kernel(PtLensArgs a0) {
    pt_shade_frame<MODE, TEX, PARK, PtLensPass>(a0);
}

hipError_t PT_INST_CAT(pt_lens_launch_mode_, PT_INST_MODE)(const PtLensArgs& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    return pt_shade_launch<PT_INST_MODE, PtLensPass>(a, tex, park, n_cu, stream, grid, launch);
}
