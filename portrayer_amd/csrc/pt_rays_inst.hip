// One traversal mode's instantiation of pt_rays_kernel (pt_rays.h) and its launcher. Compiled once per mode, -DPT_INST_MODE=1..9
// (Makefile: pt_rays_m<mode>.o), beside the render kernels' objects and through the same check / repair of the assembly.
#include "pt_rays.h"

#ifndef PT_INST_MODE
#error "compile with -DPT_INST_MODE=<PT_MODE_*>"
#endif
#define PT_INST_CAT2(a, b) a##b
#define PT_INST_CAT(a, b) PT_INST_CAT2(a, b)

hipError_t PT_INST_CAT(pt_rays_launch_mode_, PT_INST_MODE)(const PtRaysArgs& a, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    return pt_rays_launch<PT_INST_MODE>(a, n_cu, stream, grid, launch);
}
