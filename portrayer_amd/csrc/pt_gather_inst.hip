// One traversal mode's instantiations of pt_gather_kernel (pt_gather.h) and their launcher. Compiled once per mode, -DPT_INST_MODE=1..9
// (Makefile: pt_gather_m<mode>.o), beside the radiance pass's and the film's objects and through the same check / repair of the assembly.
#include "pt_gather.h"

#ifndef PT_INST_MODE
#error "compile with -DPT_INST_MODE=<PT_MODE_*>"
#endif
#define PT_INST_CAT2(a, b) a##b
#define PT_INST_CAT(a, b) PT_INST_CAT2(a, b)

hipError_t PT_INST_CAT(pt_gather_launch_mode_, PT_INST_MODE)(const PtGatherArgs& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    return pt_shade_launch<PT_INST_MODE, PtGatherPass>(a, tex, park, n_cu, stream, grid, launch);
}
