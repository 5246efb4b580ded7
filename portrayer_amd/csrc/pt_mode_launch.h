// One launcher per traversal mode and pass: <prefix>n, n = 1 .. 9, each defined in an object of its own (the pass's _inst.hip compiled with
// -DPT_INST_MODE=n) so that the nine sets of kernel instantiations compile side by side. Shared by every *_inst.h: the nine declarations of a pass,
// and the one place that says which PT_MODE_* (pt_scene_view.h) is which n.
#pragma once

#include <hip/hip_runtime.h>

// PT_DECLARE_MODE_LAUNCHERS(pt_aov_launch_mode_, const PtAovArgs& a, ...): the launchers of one pass, all with the parameter list that follows the prefix.
#define PT_DECLARE_MODE_LAUNCHERS(prefix, ...) \
    hipError_t prefix##1(__VA_ARGS__);         \
    hipError_t prefix##2(__VA_ARGS__);         \
    hipError_t prefix##3(__VA_ARGS__);         \
    hipError_t prefix##4(__VA_ARGS__);         \
    hipError_t prefix##5(__VA_ARGS__);         \
    hipError_t prefix##6(__VA_ARGS__);         \
    hipError_t prefix##7(__VA_ARGS__);         \
    hipError_t prefix##8(__VA_ARGS__);         \
    hipError_t prefix##9(__VA_ARGS__)

// PT_MODE_LAUNCH(pt_aov_launch_mode_, mode, a, ...): the body of a function that forwards its arguments to the launcher of `mode`. PT_MODE_FLAT is 1, the default.
#define PT_MODE_LAUNCH(prefix, mode, ...)                            \
    switch (mode) {                                                  \
    case PT_MODE_KD: return prefix##2(__VA_ARGS__);                  \
    case PT_MODE_FLAT_NOMESH: return prefix##3(__VA_ARGS__);         \
    case PT_MODE_FLAT_KDMESH: return prefix##4(__VA_ARGS__);         \
    case PT_MODE_HIER: return prefix##5(__VA_ARGS__);                \
    case PT_MODE_HIER_NOMESH: return prefix##6(__VA_ARGS__);         \
    case PT_MODE_KD_NOMESH: return prefix##7(__VA_ARGS__);           \
    case PT_MODE_HIER_MESH: return prefix##8(__VA_ARGS__);           \
    case PT_MODE_KD_MESH: return prefix##9(__VA_ARGS__);             \
    default: return prefix##1(__VA_ARGS__);                          \
    }
