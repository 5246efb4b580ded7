// One traversal mode's instantiations of pt_film_map_kernel (pt_film_map.h) and their launcher. Compiled once per mode, -DPT_INST_MODE=1..9
// (Makefile: pt_film_map_m<mode>.o), beside the film's objects and through the same check / repair of the assembly.
#include "pt_film_map.h"

#ifndef PT_INST_MODE
#error "compile with -DPT_INST_MODE=<PT_MODE_*>"
#endif
#define PT_INST_CAT2(a, b) a##b
#define PT_INST_CAT(a, b) PT_INST_CAT2(a, b)

hipError_t PT_INST_CAT(pt_film_map_launch_mode_, PT_INST_MODE)(const PtFilmMapArgs& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    return pt_shade_launch<PT_INST_MODE, PtFilmMapPass>(a, tex, park, n_cu, stream, grid, launch);
}
