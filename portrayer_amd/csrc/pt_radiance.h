// The radiance pass (pt_radiance, include/portrayer_hip.h): rays the CALLER supplies - origin and direction in world space, as in the ray-query pass
// (pt_rays.h) - and per ray the bits of Ray::color(scene, background_i, 0) (ray.rs:139-148): Blinn-Phong with shadow rays, area lights, glossy reflection,
// reflection and refraction to depth 10, textures and normal maps. One shaded sample per ray, linear f64: no mean, no gamma, no clamp.
//
// Work item: one wavefront = 64 consecutive ray indices, or with a permutation (reorder = 1, pt_rays_sort.hip) 64 consecutive entries of it. Each lane
// carries its ray's INDEX: the ray, its background colour and its result are read and written through it, and so are its random draws - stream
// (seed, stream_base + index, sample), draws 2, 3, ... as the render numbers them behind its two jitter draws (PtRaySource, pt_radiance_inst.h). So no result
// depends on which rays share a wavefront or on the order they are taken in.
//
// Nothing of the shading is new: every lane runs the render's interpreter (pt_lane_advance, pt_shade.h; restated below with a source policy) to the end of its
// sample, all 64 lanes meeting in the one pt_trace_wave<MODE> per pass whatever kind of ray each carries, as in pt_render_kernel. What differs is the source and the end of an item: the
// lane writes its own `value` to rgb[index]. Rays that are not traced (pt_rays_traced) carry no ray and report their background colour.
// No counting variant, no fork / join, no occluder table (that one belongs to a render's tiles).
//
// LDS of a block as in pt_render_kernel: the traversal stack area, the hit frame per lane, and (PARK = 1) the youngest parked recursion frame per lane; older
// frames in the lane's own 128-byte lines in HBM (PtRenderArgs::spill). Persistent wavefronts, one item at a time from 16 interleaved queues. This is the
// shading passes' frame: pt_shade_frame.h holds it for the film's kernels, this kernel keeps its own copy because on the shared frame four of
// its instantiations spill differently. The launcher and the re-read of the argument block are the shared ones.
#pragma once

#include "pt_shade_frame.h"
#include "pt_radiance_inst.h"

// ------------------------------------------------------------------------------------------------
// The interpreter with a SOURCE. pt_source_advance and pt_source_light_position are pt_lane_advance and pt_light_position (pt_shade.h) restated line for
// line - the same expressions in the same order, so the same bits - with one difference: where the render's text reads the camera, the lane's pixel, the
// item's sample index and the background image, these ask a compile-time policy SRC:
//   src.primary(a, L)      the lane's primary ray                       (render: pt_camera_ray through the pixel, jittered by draws 0 and 1)
//   src.background(a, L)   the colour a miss and a depth-11 ray return  (render: pt_background at the pixel)
//   src.sample(a, L), src.stream(a, L)   second and third word of the generator's counter for draws 2, 3, ...   (render: the item's sample, y * width + x)
// They are a copy, not a template parameter of the originals, because the render kernels' code objects are to stay byte-identical to what they were and
// hipcc's output for them changes (instruction order, operand order of commutative operations; no more) with ANY edit of the templates they instantiate,
// a defaulted policy parameter included. A change of pt_lane_advance must be made here too; tests/test_gpu_radiance.py compares the two bit for bit on
// every example scene (radiance of the pixel-centre rays == pt_render's linear buffer).
// ------------------------------------------------------------------------------------------------
template <class SRC>
PT_HD PtVec3 pt_source_light_position(const PtRenderArgs& a, const PtLane& L, const double* light, uint32_t draw0, bool* is_area, const SRC& src) {
    PtVec3 pos = pt_v3(light[0], light[1], light[2]);
    PtVec3 aa = pt_v3(light[9], light[10], light[11]), ab = pt_v3(light[12], light[13], light[14]);
    bool empty = (aa.x == 0.0 && aa.y == 0.0 && aa.z == 0.0) || (ab.x == 0.0 && ab.y == 0.0 && ab.z == 0.0);  // light.rs:51-53
    *is_area = !empty;
    if (empty) return pos;
    const uint32_t sample = src.sample(a, L);
    uint64_t pixel = src.stream(a, L);
    double a_coord = 2.0 * pt_rng_f64(a.seed, pixel, sample, draw0) - 1.0;
    double b_coord = 2.0 * pt_rng_f64(a.seed, pixel, sample, draw0 + 1) - 1.0;
    return pos + (aa * a_coord + ab * b_coord);
}

template <bool TEX, bool HIER, int PARK, class SRC>
PT_HD void pt_source_advance(const PtRenderArgs& a, PtLane& L, const PtHit& hit, const PtFrameRef& fr, PtCounters* cnt, uint32_t pre, const SRC& src) {
    constexpr bool STATS = false, FORK = false;  // no counting variant, no fork / join: those branches of the render's text compile out
    const PtSceneView& sc = a.scene;
    L.has_ray = false;
    PtVec3 value = pt_v3(0.0, 0.0, 0.0);  // colour being returned to the parent frame
    bool returning = false;
    for (;;) {
        if (returning) {
            // `value` = Ray::color() of the ray cast at depth L.depth
            returning = false;
            if (FORK && L.depth == L.base && L.base > 0) {  // a taken subtree is finished: its colour to the owner's mailbox, then the ticket
                double* mail = fr.spill + ((ptrdiff_t)(int32_t)(L.owner & 0xFFFFu) - (ptrdiff_t)PT_THREAD_IN_BLOCK()) * (PT_SPILL_DEPTHS * PT_SPILL_STRIDE) +
                               (size_t)(L.owner >> 16) * PT_SPILL_STRIDE + PT_H_MAIL;
                mail[0] = value.x; mail[1] = value.y; mail[2] = value.z;
                pt_mail_store(mail + 3, L.ticket);
                L.base = 0;
                L.stage = PT_ST_DONE;
                return;
            }
            if (L.depth == 0) {  // render.rs:36-43: this sample's colour, summed with its chunk by pt_render_kernel
                if (FORK) fr.set_h3(PT_RESULT_DEPTH, PT_H_MAIL, value);  // the LDS frame is reused by the tasks this lane may take
                else fr.set_l3(PT_L_VALUE, value);
                L.stage = PT_ST_DONE;
                return;
            }
            L.depth--;
            double f[PT_PARK_F64];
            const bool in_lds = PARK > 0 && L.depth >= L.lo;
            if (in_lds) fr.load_lds(0, f);
            else { fr.load_hbm(L.depth, f); if (PARK > 0) L.lo = L.depth; }  // nothing younger can be parked: the LDS slot is free
            uint32_t mat, fstage;
            PtFrameRef::unpack_tag(f[PT_H_TAG], &mat, &fstage);
            const double reflectivity = f[PT_H_REFL];
            PtVec3 color = pt_v3(f[PT_H_COLOR], f[PT_H_COLOR + 1], f[PT_H_COLOR + 2]);
            if ((fstage & PT_FS_STAGE_MASK) == PT_FS_WAIT_REFRACT) {  // material.rs:305-309
                PtVec3 reflected = pt_v3(f[PT_H_DIR], f[PT_H_DIR + 1], f[PT_H_DIR + 2]);
                double schlick = f[PT_H_SCHLICK];
                double transmittance = 1.0 - schlick;
                PtVec3 total = reflected * schlick + value * transmittance;
                value = color + total * reflectivity;
                returning = true;
                continue;
            }
            // PT_FS_WAIT_REFLECT: `value` is reflected_color (material.rs:242-243)
            if (!(fstage & PT_FS_HAVE_REFRACT)) {  // opaque (material.rs:312-316) or total internal reflection (:277-284)
                value = color + value * reflectivity;
                returning = true;
                continue;
            }
            // the refracted ray (material.rs:286-303); its direction was worked out when the hit was shaded
            const bool forked = FORK && (fstage & PT_FS_FORKED);
            if (!forked) {
                L.ray.o = pt_v3(f[PT_H_P], f[PT_H_P + 1], f[PT_H_P + 2]);
                L.ray.d = pt_v3(f[PT_H_DIR], f[PT_H_DIR + 1], f[PT_H_DIR + 2]);
            }
            // the frame waits again, now for the refracted subtree, with the reflected colour in place of the direction
            const double tag2 = PtFrameRef::pack_tag(mat, PT_FS_WAIT_REFRACT);
            if (in_lds) {
                fr.p(0, PT_H_DIR) = value.x; fr.p(0, PT_H_DIR + 1) = value.y; fr.p(0, PT_H_DIR + 2) = value.z;
                fr.p(0, PT_H_TAG) = tag2;
            } else if (PARK > 0) {  // it came from HBM and the LDS slot is free: it need not go back
                f[PT_H_DIR] = value.x; f[PT_H_DIR + 1] = value.y; f[PT_H_DIR + 2] = value.z; f[PT_H_TAG] = tag2;
                fr.store_lds(0, f);
            } else {
                fr.set_h3(L.depth, PT_H_DIR, value);
                fr.h(L.depth, PT_H_TAG) = tag2;
            }
            L.depth++;
            if (forked) {  // another lane walks that subtree: wait for its colour (the ticket in this frame's mailbox)
                L.wait_ticket = pt_fork_ticket(a.launch_nonce, fstage >> PT_FS_SEQ_SHIFT, L.depth - 1);
                L.stage = PT_ST_WAIT_FORK;
                return;
            }
            L.ray_any = false; L.has_ray = true; L.stage = PT_ST_CLOSEST_DONE;
            if (STATS) cnt->refract++;
            return;
        }
        if (FORK && L.stage == PT_ST_WAIT_FORK) {
            const double* mail = fr.spill + (size_t)(L.depth - 1) * PT_SPILL_STRIDE + PT_H_MAIL;
            if (pt_mail_load(mail + 3) != L.wait_ticket) return;  // not yet: no ray this pass
            value = pt_v3(mail[0], mail[1], mail[2]);
            returning = true;  // as if the refracted ray's Ray::color() had just returned (material.rs:305-309 follows)
            continue;
        }
        switch (L.stage) {
        case PT_ST_NEW_SAMPLE: {
            PT_FENCE;
            L.ray = src.primary(a, L);
            L.draw = 2;  // draws 0 and 1 are the render's jitter, whatever the source
            L.depth = 0;
            if (PARK > 0) L.lo = 0;
            L.ray_any = false; L.has_ray = true; L.stage = PT_ST_CLOSEST_DONE;
            if (STATS) cnt->primary++;
            return;
        }
        case PT_ST_CLOSEST_DONE: {  // ray.rs:139-148
            PT_FENCE;
            if (hit.node == PT_NO_HIT) { value = src.background(a, L); returning = true; continue; }
            if (STATS) cnt->hits++;
            PtVec3 P, N;
            uint32_t mat, ftag;
#ifdef PT_MAPS_BEFORE
            pt_hit_surface<TEX, HIER, true, true>(sc, L.ray, hit, &P, &N, &mat, &ftag);
#else
            pt_hit_surface<TEX, HIER, false, true>(sc, L.ray, hit, &P, &N, &mat, &ftag);
#endif
            fr.set_l3(PT_L_P, P);
            PT_FENCE;
            if (TEX && (pre & PT_PRE_MAPS)) ftag = pre & (PT_FS_TEXEL | 0xFFFFFFu);  // pt_lane_maps ran for this hit
            if (!(TEX && (pre & PT_PRE_NORMAL))) fr.set_l3(PT_L_N, N);                // (else the normal map's normal is already there)
            fr.set_l3(PT_L_D, L.ray.d);
            fr.l(PT_L_TAG) = PtFrameRef::pack_tag(mat, ftag);
            L.light = 0;
            L.occluded = 0;
            L.draw0 = L.draw;
            L.stage = PT_ST_LIGHT;
            continue;
        }
        case PT_ST_LIGHT: {  // material.rs:149-179: one shadow ray per light, whatever the material
            PT_FENCE;
            if (L.light >= sc.n_lights) { L.stage = PT_ST_SHADE; continue; }  // a scene without lights
            const double* light = sc.lights + 15 * (size_t)L.light;
            bool is_area;
            PtVec3 lpos = pt_source_light_position(a, L, light, L.draw, &is_area, src);
            if (is_area) L.draw += 2;
            PtVec3 P = fr.l3(PT_L_P);
            PtVec3 hit_to_light = lpos - P;
            double light_dist = pt_length(hit_to_light);
            L.ray.o = P;
            L.ray.d = hit_to_light / light_dist;
            L.ray_any = true; L.has_ray = true; L.stage = PT_ST_SHADOW_DONE;
            if (STATS) cnt->shadow++;
            return;
        }
        case PT_ST_SHADOW_DONE: {  // material.rs:174-179 only asks whether anything is in the way
            if (hit.node != PT_NO_HIT) L.occluded |= 1u << (L.light % PT_LIGHT_ROUND);
            L.light++;
            L.stage = (L.light >= sc.n_lights || L.light % PT_LIGHT_ROUND == 0) ? PT_ST_SHADE : PT_ST_LIGHT;
            continue;
        }
        default: {  // PT_ST_SHADE: material.rs:148-243 for the lights whose shadow rays are back
            PT_FENCE;
            uint32_t mat, ftag;
            PtFrameRef::unpack_tag(fr.l(PT_L_TAG), &mat, &ftag);
            const double* m = sc.materials + 10 * (size_t)mat;
            PtVec3 ray_dir = fr.l3(PT_L_D), P = fr.l3(PT_L_P), N = fr.l3(PT_L_N);
            PtVec3 kd = pt_v3(m[0], m[1], m[2]), ks = pt_v3(m[3], m[4], m[5]);
            if (TEX && (ftag & PT_FS_TEXEL)) kd = pt_v3(sc.srgb_lut[ftag & 255u], sc.srgb_lut[(ftag >> 8) & 255u], sc.srgb_lut[(ftag >> 16) & 255u]);
            const uint32_t round_first = (L.light - 1u) / PT_LIGHT_ROUND * PT_LIGHT_ROUND;  // L.light > 0 here unless the scene has no light
            PtVec3 color;
            if (sc.n_lights == 0 || round_first == 0) color = pt_v3(sc.ambient[0], sc.ambient[1], sc.ambient[2]) * kd;  // material.rs:148
            else color = fr.h3(L.depth, PT_H_COLOR);  // a later round of a scene with > 32 lights
            uint32_t draw = L.draw0;
            for (uint32_t li = sc.n_lights ? round_first : 0u; li < L.light; li++) {  // material.rs:179-210
                const double* light = sc.lights + 15 * (size_t)li;
                bool is_area;
                PtVec3 lpos = pt_source_light_position(a, L, light, draw, &is_area, src);
                if (is_area) draw += 2;
                if ((L.occluded >> (li - round_first)) & 1u) continue;
                PtVec3 hit_to_light = lpos - P;
                double light_dist = pt_length(hit_to_light);
                PtVec3 light_dir = hit_to_light / light_dist;
                color = color + pt_light_term(pt_v3(light[3], light[4], light[5]), pt_v3(light[6], light[7], light[8]), light_dir, light_dist, N, ray_dir, kd, ks, m[6]);
            }
            if (L.light < sc.n_lights) {  // more than 32 lights: park the colour and do the next 32
                fr.set_h3(L.depth, PT_H_COLOR, color);
                L.occluded = 0;
                L.draw0 = L.draw;
                L.stage = PT_ST_LIGHT;
                continue;
            }
            PT_FENCE;
            // material.rs:216-243
            const double reflectivity = m[7], glossy = m[8], ior = m[9];
            if (!(reflectivity > 0.0)) { value = color; returning = true; continue; }
            PtVec3 reflect_dir = ray_dir - (N * 2.0) * pt_dot(ray_dir, N);  // material.rs:218
            if (glossy > 0.0) {  // material.rs:221-239 (not renormalised: quirk Q5)
                PtVec3 off = (fabs(reflect_dir.x) < PT_EPSILON && fabs(reflect_dir.y) < PT_EPSILON)
                                 ? reflect_dir + pt_v3(0.0, 0.1, 0.0) : reflect_dir + pt_v3(0.0, 0.0, 0.1);
                PtVec3 u_basis = pt_cross(reflect_dir, off);
                PtVec3 v_basis = pt_cross(reflect_dir, u_basis);
                const uint32_t sample = src.sample(a, L);
                uint64_t pixel = src.stream(a, L);
                double u_coord = -glossy / 2.0 + pt_rng_f64(a.seed, pixel, sample, L.draw) * glossy;
                double v_coord = -glossy / 2.0 + pt_rng_f64(a.seed, pixel, sample, L.draw + 1) * glossy;
                L.draw += 2;
                reflect_dir = reflect_dir + (u_basis * u_coord + v_basis * v_coord);
            }
            // The refracted ray (material.rs:245-303) is cast after the reflected subtree has returned; its direction and
            // the Schlick term depend only on this hit, so they are worked out now and parked with the frame.
            PtVec3 refract_dir = pt_v3(0.0, 0.0, 0.0);
            double schlick = 0.0;
            bool have = false;
            if (ior > 0.0) {
                double cos_incident = 0.0;
                if (pt_dot(ray_dir, N) < 0.0) {  // entering (material.rs:253-265)
                    if (pt_refracted_direction(ray_dir, N, ior, &refract_dir)) { cos_incident = pt_dot(-ray_dir, N); have = true; }
                } else if (pt_refracted_direction(ray_dir, -N, 1.0 / ior, &refract_dir)) {  // leaving (:266-276)
                    cos_incident = pt_dot(refract_dir, N); have = true;
                }
                // !have: total internal reflection (:277-284); also where the reference's expect() at :257-258 would panic
                if (have) {
                    double r0 = (ior - 1.0) * (ior - 1.0);
                    r0 = r0 / ((ior + 1.0) * (ior + 1.0));
                    schlick = r0 + (1.0 - r0) * pt_powi5(1.0 - cos_incident);
                }
            }
            if (L.depth + 1 > PT_MAX_DEPTH) {  // depth-11 rays: their colour is always the background (material.rs:102-104), not traced
                if (STATS) cnt->depth11_skipped++;
                PtVec3 bg = src.background(a, L);
                if (!have) {
                    value = color + bg * reflectivity;
                } else {
                    if (STATS) cnt->depth11_skipped++;
                    double transmittance = 1.0 - schlick;
                    PtVec3 total = bg * schlick + bg * transmittance;
                    value = color + total * reflectivity;
                }
                returning = true;
                continue;
            }
            {
                double f[PT_PARK_F64];
                f[PT_H_COLOR] = color.x; f[PT_H_COLOR + 1] = color.y; f[PT_H_COLOR + 2] = color.z;
                uint32_t fs = PT_FS_WAIT_REFLECT | (have ? PT_FS_HAVE_REFRACT : 0);
                if (FORK && have) {  // the refracted ray may be taken by an idle lane (pt_render_kernel matches offers and takers)
                    L.fork_seq++;
                    fs |= L.fork_seq << PT_FS_SEQ_SHIFT;
                    L.offer = true;
                    // whatever an earlier launch (of this or another process) left in this frame's mailbox must not pass for a
                    // ticket: cleared here, by the owner, passes before any taker can write it
                    pt_mail_store(&fr.h(L.depth, PT_H_MAIL_TICKET), 0ull);
                }
                f[PT_H_TAG] = PtFrameRef::pack_tag(mat, fs);
                f[PT_H_DIR] = refract_dir.x; f[PT_H_DIR + 1] = refract_dir.y; f[PT_H_DIR + 2] = refract_dir.z;
                f[PT_H_P] = P.x; f[PT_H_P + 1] = P.y; f[PT_H_P + 2] = P.z;
                f[PT_H_SCHLICK] = schlick;
                f[PT_H_REFL] = reflectivity;
                if (PARK > 0) {
                    if (L.depth - L.lo == 1) {  // the LDS slot holds the parent's frame: that one goes to its HBM line
                        double old[PT_PARK_F64];
                        fr.load_lds(0, old);
                        fr.store_hbm(L.lo, old);
                        L.lo++;
                    }
                    fr.store_lds(0, f);
                } else {
                    fr.store_hbm(L.depth, f);
                }
            }
            L.ray.o = P;
            L.ray.d = reflect_dir;
            L.depth++;
            L.ray_any = false; L.has_ray = true; L.stage = PT_ST_CLOSEST_DONE;
            if (STATS) cnt->reflect++;
            return;
        }
        }
    }
}

template <int MODE, bool TEX, int PARK>
__global__ void __launch_bounds__(PT_BLOCK, pt_radiance_waves(MODE)) pt_radiance_kernel(PtRadianceArgs a0) {
    constexpr bool HIER = MODE == PT_MODE_HIER || MODE == PT_MODE_HIER_NOMESH || MODE == PT_MODE_HIER_MESH;
    extern __shared__ uint32_t pt_lds[];
    const PtRenderArgs& a = a0.r;
    const uint32_t lane_global = blockIdx.x * PT_BLOCK + threadIdx.x;
    const unsigned lane = threadIdx.x & 63u;
    PtStackSpill stk;
    stk.base = pt_lds + threadIdx.x;
    stk.cap = a.stack_lds_cap;
    stk.total = a.scene.stack_cap;
    stk.gbase = a.stack_spill + lane_global;
    stk.gstride = a.n_lanes;
    stk.overflow = a.overflow_flag;
    PtFrameRef fr;
    fr.lds = reinterpret_cast<double*>(pt_lds + (size_t)a.stack_lds_cap * PT_BLOCK) + threadIdx.x;
    fr.park = fr.lds + (size_t)PT_LDS_FRAME_F64 * PT_FRAME_STRIDE;
    fr.spill = a.spill + (size_t)lane_global * (PT_SPILL_DEPTHS * PT_SPILL_STRIDE);
    fr.n_lanes = a.n_lanes;
    PtCounters cnt;  // (the walks and the interpreter take a pointer; nothing is counted)
    PtLane L;
    L.stage = PT_ST_DONE; L.has_ray = false; L.ray_any = false;
    L.item = 0; L.x = L.y = 0; L.light = L.draw = L.draw0 = L.occluded = 0; L.depth = 0; L.lo = 0;
    L.ray.o = L.ray.d = pt_v3(0.0, 0.0, 0.0);
    L.offer = false; L.base = 0; L.owner = 0; L.fork_seq = 0; L.ticket = 0; L.wait_ticket = 0;
    PtHit hit;
    hit.t = INFINITY; hit.node = PT_NO_HIT; hit.sub = 0;

    // items are handed out one at a time from interleaved queues (pt_rays_kernel, pt_render_kernel): item idx * N + q from queue q
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
        const uint64_t slot = (uint64_t)w * 64u + lane;
        const bool mine = slot < a0.n;
        uint32_t i = (uint32_t)slot;                  // (n <= PT_RAYS_MAX = 2^30)
        if (mine && a0.perm) i = a0.perm[slot];       // (< n: a permutation of 0 .. n - 1)
        PtRay ray;
        ray.o = ray.d = pt_v3(0.0, 0.0, 0.0);
        if (mine) {
            const double* o = a0.origins + 3 * (size_t)i;
            const double* d = a0.directions + 3 * (size_t)i;
            ray.o = pt_v3(o[0], o[1], o[2]);
            ray.d = pt_v3(d[0], d[1], d[2]);
        }
        const bool traced = mine && pt_rays_traced(ray);
        if (mine && !traced) {  // not traced: its own background colour, and no part in anything below
            const double* b = a0.background + (size_t)a0.bg_stride * i;
            double* o = a0.rgb + 3 * (size_t)i;
            o[0] = b[0]; o[1] = b[1]; o[2] = b[2];
        }
        if (!traced) ray.o = ray.d = pt_v3(0.0, 0.0, 0.0);  // what an idle lane of the render kernels holds: no NaN reaches the walk's arithmetic
        L.item = w;
        L.x = traced ? i : 0u;  // the ray's index: what the source policy reads the background and the stream through
        L.ray = ray;
        L.stage = traced ? PT_ST_NEW_SAMPLE : PT_ST_DONE;
        L.has_ray = false;
        for (;;) {
            const bool active = L.stage != PT_ST_DONE;
            if (!__any(active)) break;
            // what the interpreter and this pass's walk need of the arguments is fetched now, not kept from the top of the kernel on (pt_render_kernel)
            const PtRadianceArgs& aa = pt_args_again(a0);
            const PtRenderArgs& a = aa.r;
            PtRaySource src;
            src.bg = aa.background; src.bg_stride = aa.bg_stride; src.sample_index = aa.sample; src.stream_base = aa.stream_base;
            if (active) pt_source_advance<TEX, HIER, PARK, PtRaySource>(a, L, hit, fr, &cnt, 0u, src);
            const bool tracing = L.stage != PT_ST_DONE && L.has_ray;
            if (__any(tracing)) pt_trace_wave<MODE, false>(a, L.ray, tracing, L.ray_any, hit, stk, pt_lds, &cnt);
        }
        // the lane's own finished sample, out of its own LDS column (same lane: program order suffices), to its ray's place: its index is still in L.x
        // (the interpreter never writes it)
        if (traced) {
            const PtVec3 value = fr.l3(PT_L_VALUE);
            double* o = a0.rgb + 3 * (size_t)L.x;
            o[0] = value.x; o[1] = value.y; o[2] = value.z;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// What pt_shade_launch (pt_shade_frame.h) asks of a pass
struct PtRadiancePass {
    using Args = PtRadianceArgs;
    static PT_HD const PtRenderArgs& render(const PtRadianceArgs& a0) { return a0.r; }
    template <int MODE, bool TEX, int PARK>
    static constexpr auto kernel() { return &pt_radiance_kernel<MODE, TEX, PARK>; }
};
