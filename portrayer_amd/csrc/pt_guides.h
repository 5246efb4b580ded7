// The guides pass (pt_guides, include/portrayer_hip.h): ONE primary ray per pixel of the slice and what a denoiser needs of its hit - the
// diffuse colour under the pixel (albedo), the world-space point, the normalised world-space normal and the flattened node - in one trace. No shading, no
// lights, no secondary rays, no random numbers.
//
// It is the primary-visibility pass (pt_aov.h) with one more output: the same ray (pt_camera_ray at (x + offset.x, y + offset.y)), the same nearest hit over
// [PT_EPSILON, inf) by pt_trace_wave, the same work distribution (a wavefront = one 8x8 tile, persistent wavefronts, 16 interleaved queues), and position,
// normal and node in that pass's bits with its miss values. The normal is the one BEFORE any normal map, as there.
//
// albedo: material.rs:137-143's diffuse_color at the hit, in the bits the render path uses - the material record's diffuse, or, where the material has a
// texture, srgb_lut[] of the texel's three bytes, the texel fetched at uv_trans * uv as pt_apply_maps fetches it: the kd pt_shade.h forms from the hit's texel tag in
// front of its light loop. (+0, +0, +0) on a miss.
//
// TEX = false (scenes without maps) reads the material record only. TEX = true rebuilds the model-space hit (pt_hit_model, as pt_hit_surface does) and
// calls the out-of-line pt_guides_texel for materials with a texture; a material with a normal map alone does not: nothing of that map is an output here.
#pragma once

#include "pt_render_kernel.h"
#include "pt_guides_inst.h"

// The texel tag (PtMapsOut::texel) of a hit on a material with a texture: the uv of pt_apply_maps_body (pt_shade.h) - the same expressions in the same order,
// so the same bits - times uv_trans, and the texel there. Restated, not called: pt_apply_maps also builds the tangent frame a normal map needs, which is no
// output here, and indexes its cube tables in scratch memory (112 bytes per lane); this routine has neither, so that no instantiation of a mesh-free mode
// touches scratch. Out of line (PT_GUIDES_TEXEL_ATTR), as pt_apply_maps is, so that the code around the call keeps its registers.
// type / sub / local identify the hit, p and n are its model-space point and raw normal (pt_hit_model).
#ifndef PT_GUIDES_TEXEL_ATTR
#define PT_GUIDES_TEXEL_ATTR PT_NOINLINE
#endif
PT_GUIDES_TEXEL_ATTR uint32_t pt_guides_texel(const PtTexView* view, uint32_t mat, uint32_t type, uint32_t sub, double ox, double oy, double oz, double dx, double dy, double dz, double px,
                                              double py, double pz, double nx, double ny, double nz) {
    const int32_t tex_id = view->mat_maps[2 * mat];
    const double* uv_trans9 = view->uv_trans + 9 * (size_t)mat;
    const PtVec3 p = pt_v3(px, py, pz), fn = pt_v3(nx, ny, nz);
    double u = 0.0, v = 0.0;
    if (type == PT_SPHERE) {  // sphere.rs:53-61
        const double PI = 3.14159265358979323846;
        u = (PI + atan2(-p.z, p.x)) / (2.0 * PI);
        v = acos(p.y) / PI;
    } else if (type == PT_CUBE) {  // cube.rs:46-66, :84-112; sub = the face, the tables of pt_apply_maps_body as selects
        const double ax_u = (sub == 0u || sub == 5u) ? -1.0 : 1.0, ax_v = sub == 2u ? -1.0 : 1.0;
        const double off_u = sub == 0u ? 1.0 / 2.0 : (sub == 1u ? 0.0 : (sub == 5u ? 3.0 / 4.0 : 1.0 / 4.0));
        const double off_v = sub == 2u ? 0.0 : (sub == 3u ? 2.0 / 3.0 : 1.0 / 3.0);
        double fu, fv;
        if (fn.x != 0.0) { fu = p.z; fv = p.y; } else if (fn.y != 0.0) { fu = p.x; fv = p.z; } else { fu = p.x; fv = p.y; }
        double nu = fu * ax_u + 0.5, nv = 0.5 - fv * ax_v;
        u = nu / 4.0 + off_u;
        v = nv / 3.0 + off_v;
    } else if (type == PT_PLANE) {  // plane.rs:40-46
        u = p.x + 0.5; v = p.z + 0.5;
    } else {  // triangle with texture coordinates: triangle.rs:90-138
        const double* tv = view->tri_v + 9 * (size_t)sub;
        const double* q = view->tri_uv + 6 * (size_t)sub;
        PtRay local; local.o = pt_v3(ox, oy, oz); local.d = pt_v3(dx, dy, dz);
        double t2, beta, gamma;
        pt_triangle_hit(tv, local, -INFINITY, INFINITY, &t2, &beta, &gamma);
        double alpha = 1.0 - beta - gamma;
        double uu = (q[0] * alpha + q[2] * beta) + q[4] * gamma, vv = (q[1] * alpha + q[3] * beta) + q[5] * gamma;
        u = uu; v = 1.0 - vv;
    }
    // material.rs:113-117: uv_trans * (u, v, 1)
    double tu = (uv_trans9[0] * u + uv_trans9[1] * v) + uv_trans9[2] * 1.0;
    double tv2 = (uv_trans9[3] * u + uv_trans9[4] * v) + uv_trans9[5] * 1.0;
    PtVec3 c = pt_texel(view->tex, view->tex_rgb, tex_id, tu, tv2);  // texture.rs:162-168
    return PT_FS_TEXEL | (uint32_t)(int)c.x | ((uint32_t)(int)c.y << 8) | ((uint32_t)(int)c.z << 16);
}

template <int MODE, bool TEX>
__global__ void __launch_bounds__(PT_BLOCK, pt_aov_waves(MODE)) pt_guides_kernel(PtGuidesArgs a0) {
    constexpr bool HIER = MODE == PT_MODE_HIER || MODE == PT_MODE_HIER_NOMESH || MODE == PT_MODE_HIER_MESH;
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

    // tiles from the interleaved queues, as in pt_aov_kernel: tile idx * N + q from queue q
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
        if (a0.node) a0.node[px] = ok ? (int32_t)hit.node : -1;
        if (a0.position || a0.normal) {  // (wave-uniform: no world transform is computed that nobody asked for)
            PtVec3 P = pt_v3(0.0, 0.0, 0.0), N = P;
            if (ok) {
                uint32_t mat, ftag;
                pt_hit_surface<false, HIER>(sc, ray, hit, &P, &N, &mat, &ftag);
            }
            if (a0.position) { double* o = a0.position + 3 * px; o[0] = P.x; o[1] = P.y; o[2] = P.z; }
            if (a0.normal) { double* o = a0.normal + 3 * px; o[0] = N.x; o[1] = N.y; o[2] = N.z; }
        }
        if (a0.albedo) {
            PtVec3 kd = pt_v3(0.0, 0.0, 0.0);
            if (ok) {
                const uint32_t mat = sc.info[4 * (size_t)hit.node + 3];
                const double* m = sc.materials + 10 * (size_t)mat;
                kd = pt_v3(m[0], m[1], m[2]);
                if (TEX && sc.mat_maps && sc.mat_maps[2 * mat] >= 0) {  // material.rs:137-143: the texel in place of the record's diffuse
                    uint32_t type, mat2;
                    PtRay local;
                    PtVec3 p, n;
                    pt_hit_model<HIER>(sc, ray, hit, &type, &mat2, &local, &p, &n);
                    const uint32_t ftag = pt_guides_texel(sc.texview, mat, type, hit.sub, local.o.x, local.o.y, local.o.z, local.d.x, local.d.y, local.d.z, p.x, p.y, p.z, n.x, n.y, n.z);
                    kd = pt_v3(sc.srgb_lut[ftag & 255u], sc.srgb_lut[(ftag >> 8) & 255u], sc.srgb_lut[(ftag >> 16) & 255u]);
                }
            }
            double* o = a0.albedo + 3 * px;
            o[0] = kd.x; o[1] = kd.y; o[2] = kd.z;
        }
    }
}

// Launch (or, with launch = false, only size) the pass: the grid is what is resident, by the render kernels' launcher (pt_launch_kernel_args).
template <int MODE>
static hipError_t pt_guides_launch(const PtGuidesArgs& a, bool tex, int n_cu, hipStream_t stream, uint32_t* grid_out, bool launch) {
    const size_t lds = (size_t)a.r.stack_lds_cap * PT_BLOCK * 4;  // the traversal stack area alone, as in pt_aov_launch
    if (tex) return pt_launch_kernel_args<&pt_guides_kernel<MODE, true>>(lds, a, a.r.n_items, a.r.grid_share, n_cu, stream, grid_out, launch);
    return pt_launch_kernel_args<&pt_guides_kernel<MODE, false>>(lds, a, a.r.n_items, a.r.grid_share, n_cu, stream, grid_out, launch);
}
