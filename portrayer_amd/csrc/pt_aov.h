// The primary-visibility pass (pt_aov, include/portrayer_hip.h): ONE primary ray per pixel of the slice and what it hit - no shading, no
// lights, no secondary rays, no random numbers.
//
//     primary ray (camera.rs:48-84) at (x + offset.x, y + offset.y)  ->  nearest hit over [PT_EPSILON, inf)  ->
//     t, flattened node, triangle inside its mesh, material index; where asked for, the world-space point and the normalised world-space
//     normal (flat_scene.rs:85-95 / scene.rs:100-112, material.rs:123-125 - BEFORE any normal map)
//
// Work item: one wavefront = one 8x8 tile of the slice, lane l = pixel (l & 7, l >> 3) of the tile (the order of pt_tile_slot_pixel); lanes outside
// the slice carry no ray, as idle lanes do in the render kernels. Nothing of the tracing is new: the walk is the render kernels' pt_trace_wave
// (pt_render_simple.h: pt_trace_packet / pt_trace_packet_mesh / pt_trace_packet_kd per mode, LDS regions laid out as for a render), the surface is
// pt_hit_surface with the material maps compiled out (TEX = false). No result of the walks depends on which rays share a wavefront, so
// a tile of neighbouring pixels gets the bits a render's samples get.
//
// Persistent wavefronts, one tile at a time from 16 interleaved queues: the lanes' HBM stack columns (PtStackSpill) are sized by the lanes RESIDENT, as in a
// render - a plain grid over the tiles of a 1920x1080 frame would need 2 M columns -, and a tile's cost varies with what is behind it.
#pragma once

#include "pt_render_kernel.h"
#include "pt_aov_inst.h"

template <int MODE>
__global__ void __launch_bounds__(PT_BLOCK, pt_aov_waves(MODE)) pt_aov_kernel(PtAovArgs a0) {
    constexpr bool HIER = MODE == PT_MODE_HIER || MODE == PT_MODE_HIER_NOMESH || MODE == PT_MODE_HIER_MESH;
    constexpr bool MESHES = !(MODE == PT_MODE_FLAT_NOMESH || MODE == PT_MODE_HIER_NOMESH || MODE == PT_MODE_KD_NOMESH);
    extern __shared__ uint32_t pt_lds[];
    const PtRenderArgs& a = a0.r;
    const PtSceneView& sc = a.scene;
    const uint32_t lane_global = blockIdx.x * PT_BLOCK + threadIdx.x;
    const unsigned lane = threadIdx.x & 63u;
    PtStackSpill stk;
    stk.base = pt_lds + threadIdx.x;
    stk.cap = a.stack_lds_cap;
    stk.total = a.scene.stack_cap;
    stk.gbase = a.stack_spill + lane_global;
    stk.gstride = a.n_lanes;
    stk.overflow = a.overflow_flag;
    PtCounters cnt;  // (the walks take a pointer; nothing is counted)

    // tiles are handed out one at a time from interleaved queues, as the render kernels hand out their items (pt_render_simple_kernel): tile idx * N + q from queue q.
    // (Not from one counter: the 32,400 atomics of a 1920x1080 frame on one address take 0.42 ms, three times the pass - profiles/aov/notes.md.)
    unsigned q_next = blockIdx.x % a.fine_queues, q_end = 0;
    for (;;) {
        unsigned w;
        for (;;) {
            unsigned idx = 0;
            if (lane == 0) idx = atomicAdd(a.work_queues + q_next * PT_QUEUE_STRIDE, 1u);
            idx = (unsigned)__builtin_amdgcn_readfirstlane((int)idx);
            const unsigned long long pos = (unsigned long long)idx * a.fine_queues + q_next;
            if (pos < a.n_items) { w = (unsigned)pos; q_end = 0; break; }
            q_next = q_next + 1u == a.fine_queues ? 0u : q_next + 1u;
            if (++q_end == a.fine_queues) { w = 0xFFFFFFFFu; break; }
        }
        if (w == 0xFFFFFFFFu) break;
        const uint32_t ty = pt_fastdiv(w, a.div_tiles_x), tx = w - ty * a.div_tiles_x.d;
        const uint32_t x = a.x0 + tx * 8u + (lane & 7u), y = a.y0 + ty * 8u + (lane >> 3);
        const bool mine = x <= a.x1 && y <= a.y1;
        PtRay ray;
        ray.o = ray.d = pt_v3(0.0, 0.0, 0.0);
        if (mine) ray = pt_camera_ray(a.cam, (double)x + a0.off_x, (double)y + a0.off_y);
        PtHit hit;
        hit.t = INFINITY; hit.node = PT_NO_HIT; hit.sub = 0;
        pt_trace_wave<MODE, false>(a, ray, mine, false, hit, stk, pt_lds, &cnt);
        if (!mine) continue;  // (an idle lane: nothing to write)

        const size_t px = (size_t)y * a.width + x;
        const bool ok = hit.node != PT_NO_HIT;
        if (a0.depth) a0.depth[px] = ok ? hit.t : INFINITY;
        if (a0.node) a0.node[px] = ok ? (int32_t)hit.node : -1;
        if (a0.sub || a0.material) {
            int32_t sub = -1, mat = -1;
            if (ok) {
                const uint32_t* info = sc.info + 4 * (size_t)hit.node;
                mat = (int32_t)info[3];
                sub = 0;
                if (MESHES && (info[0] == PT_MESH || info[0] == PT_KDMESH)) sub = (int32_t)(hit.sub - sc.meshes[info[1]].tri_first);  // hit.sub: the triangle's index over all meshes
            }
            if (a0.sub) a0.sub[px] = sub;
            if (a0.material) a0.material[px] = mat;
        }
        if (a0.position || a0.normal) {  // (wave-uniform: no world transform is computed that nobody asked for)
            PtVec3 P = pt_v3(0.0, 0.0, 0.0), N = P;
            if (ok) {
                uint32_t mat, ftag;
                pt_hit_surface<false, HIER>(sc, ray, hit, &P, &N, &mat, &ftag);
            }
            if (a0.position) { double* o = a0.position + 3 * px; o[0] = P.x; o[1] = P.y; o[2] = P.z; }
            if (a0.normal) { double* o = a0.normal + 3 * px; o[0] = N.x; o[1] = N.y; o[2] = N.z; }
        }
    }
}

// Launch (or, with launch = false, only size) the pass: the grid is what is resident, by the render kernels' launcher (pt_launch_kernel_args).
template <int MODE>
static hipError_t pt_aov_launch(const PtAovArgs& a, int n_cu, hipStream_t stream, uint32_t* grid_out, bool launch) {
    const size_t lds = (size_t)a.r.stack_lds_cap * PT_BLOCK * 4;  // the traversal stack area alone: no hit frame waits in LDS here
    return pt_launch_kernel_args<&pt_aov_kernel<MODE>>(lds, a, a.r.n_items, a.r.grid_share, n_cu, stream, grid_out, launch);
}
