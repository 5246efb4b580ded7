// One traversal mode's instantiations of pt_radiance_kernel (pt_radiance.h) and their launcher. Compiled once per mode, -DPT_INST_MODE=1..9
// (Makefile: pt_radiance_m<mode>.o), beside the render kernels' objects and through the same check / repair of the assembly.
#include "pt_radiance.h"

#ifndef PT_INST_MODE
#error "compile with -DPT_INST_MODE=<PT_MODE_*>"
#endif
#define PT_INST_CAT2(a, b) a##b
#define PT_INST_CAT(a, b) PT_INST_CAT2(a, b)

hipError_t PT_INST_CAT(pt_radiance_launch_mode_, PT_INST_MODE)(const PtRadianceArgs& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    return pt_shade_launch<PT_INST_MODE, PtRadiancePass>(a, tex, park, n_cu, stream, grid, launch);
}
