// One traversal mode's instantiations of pt_probe_kernel - the probe pass (pt_probe, include/portrayer_hip.h) - and their launcher. Compiled once
// per mode, -DPT_INST_MODE=1..9 (Makefile: pt_probe_m<mode>.o), beside the gather pass's objects and through the same check / repair of the assembly.
//
// Per probe - a position in free space, no normal - the pass answers the nine order-2 spherical-harmonic sums of S = 64 R shaded radiance samples along the
// contract's rays (pt_probe.h): sample k of probe q being, to the bit, what pt_radiance answers for that ray with the call's background and the generator's
// stream (seed, q * S + k, pass). No ray and no per-ray colour is ever in memory: 24 bytes per probe in, at most 217 out.
//
// Work item: one wavefront = (probe, round r), lane l = sample 64 r + l. Probes come in thousands, not millions: items per round fill the machine where items
// per probe would not, and the item stays the size of pt_gather_kernel's. A lane makes its ray in registers when the item starts; the lanes of an invalid probe
// (pt_probe_valid) take no part in a walk.
//
// Nothing of the shading is new: the kernel's frame is the shading passes' (pt_shade_frame.h holds it for the film's kernels, this kernel keeps its
// own copy, as pt_gather_kernel does, because on the shared frame its instantiations spill differently) around pt_source_advance with PtProbeSource
// (pt_probe_inst.h). When every lane is PT_ST_DONE each lane's sample sits in its own LDS column (PT_L_VALUE) and the column's other seven slots (PT_L_N ..
// PT_L_TAG) are dead: the lane makes its direction again from the item, writes the basis values Y1 .. Y7 into those seven and keeps Y8 in a register (Y0 is a
// constant). Behind a wavefront barrier lanes 0 .. 26 each own one (coefficient i, channel c) pair, t = 3 i + c, and add the 64 terms Y_i(d_k) rgb_k[c] from 0 in
// ascending k - Y8 broadcast from lane k's register - so the pass needs no LDS beyond the frame's. R = 1: the 27 lanes store the probe's `sh`; R > 1: the item's
// partial, which pt_probe_fold_kernel (pt_probe.hip) adds per probe in ascending round. (The slots of one k lie 2 KiB apart, on one LDS bank: turning slot i's
// columns by i, so that the lanes of one step read seven banks, was measured and changed no time - profiles/probe/notes.md - so the plain layout stays.)
#include "pt_radiance.h"
#include "pt_probe_inst.h"

#ifndef PT_INST_MODE
#error "compile with -DPT_INST_MODE=<PT_MODE_*>"
#endif
#define PT_INST_CAT2(a, b) a##b
#define PT_INST_CAT(a, b) PT_INST_CAT2(a, b)

static_assert(PT_L_VALUE == 0 && PT_LDS_FRAME_F64 == 10, "the tail keeps Y1 .. Y7 in slots 3 .. 9 of a finished lane's column, beside its colour in 0 .. 2");

// Lane k's 64 bits, in every lane (k wave-uniform)
__device__ inline unsigned long long pt_probe_lane_u64(unsigned long long u, unsigned k) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, (int)k);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), (int)k);
    return ((unsigned long long)hi << 32) | lo;
}

template <int MODE, bool TEX, int PARK>
__global__ void __launch_bounds__(PT_BLOCK, pt_probe_waves(MODE)) pt_probe_kernel(PtProbeArgs a0) {
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

    // items are handed out one at a time from interleaved queues (pt_radiance_kernel): item idx * N + q from queue q
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
        {
            const unsigned lr = a0.log2_rounds;
            const uint32_t p = w >> lr;                                // (w < n_items = n R: p < n <= 2^20)
            const uint32_t k = ((w & ((1u << lr) - 1u)) << 6) + lane;  // < S <= 1024
            const double* P = a0.positions + 3 * (size_t)p;
            PtRay ray;
            ray.o = pt_v3(P[0], P[1], P[2]);
            ray.d = pt_v3(0.0, 0.0, 0.0);
            const bool valid = (a0.sh || a0.partial) && pt_probe_valid(ray.o);  // (the same answer in every lane; only `valid` wanted: nothing to shade)
            if (valid) ray.d = pt_probe_dir(a0.set, a0.set.first_index + p, k);
            const bool traced = valid && pt_rays_traced(ray);  // (every ray of a valid probe is: |o| <= 1e18, |d| is 1 to rounding. pt_radiance's rule all the same)
            // not traced: pt_radiance's answer for such a ray is its background colour; it waits in the lane's column like a finished sample
            if (valid && !traced) fr.set_l3(PT_L_VALUE, pt_v3(a0.background[0], a0.background[1], a0.background[2]));
            if (!traced) ray.o = ray.d = pt_v3(0.0, 0.0, 0.0);  // what an idle lane of the render kernels holds: no NaN reaches the walk's arithmetic
            L.item = w;
            L.x = traced ? p : 0u;  // the probe's index in the launch and the sample: what the source policy works the stream out from
            L.y = traced ? k : 0u;
            L.ray = ray;
            L.stage = traced ? PT_ST_NEW_SAMPLE : PT_ST_DONE;
            L.has_ray = false;
        }
        for (;;) {
            const bool active = L.stage != PT_ST_DONE;
            if (!__any(active)) break;
            // what the interpreter and this pass's walk need of the arguments is fetched now, not kept from the top of the kernel on (pt_render_kernel)
            const PtProbeArgs& aa = pt_args_again(a0);
            const PtRenderArgs& a = aa.r;
            PtProbeSource src;
            src.first_index = aa.set.first_index; src.samples = aa.samples; src.pass = aa.set.pass;
            src.bg = pt_v3(aa.background[0], aa.background[1], aa.background[2]);
            if (active) pt_source_advance<TEX, HIER, PARK, PtProbeSource>(a, L, hit, fr, &cnt, 0u, src);
            const bool tracing = L.stage != PT_ST_DONE && L.has_ray;
            if (__any(tracing)) pt_trace_wave<MODE, false>(a, L.ray, tracing, L.ray_any, hit, stk, pt_lds, &cnt);
        }
        // Every lane's finished sample is in slots 0 .. 2 of its own LDS column. The probe, the round and the lane's direction are worked out again from the item
        // (pt_render_kernel's w_again: the empty asm keeps the compiler from carrying the first computation through the walks in registers).
        unsigned w_again = w;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+s"(w_again));
#endif
        const PtProbeArgs& ab = pt_args_again(a0);
        const uint32_t p_again = w_again >> ab.log2_rounds;
        const uint32_t r_again = w_again & ((1u << ab.log2_rounds) - 1u);
        const double* P = ab.positions + 3 * (size_t)p_again;
        const bool valid_again = pt_probe_valid(pt_v3(P[0], P[1], P[2]));  // (wave-uniform)
        const bool shaded = valid_again && (ab.sh || ab.partial);
        double Y[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (shaded) {
            pt_probe_basis(pt_probe_dir(ab.set, ab.set.first_index + p_again, (r_again << 6) + lane), Y);
#pragma unroll
            for (int i = 1; i <= 7; i++) fr.l(2 + i) = Y[i];
        }
        // lanes 0 .. 26 read their neighbours' columns: same wavefront, so a wavefront barrier between the writes and the reads (pt_gather_kernel's sum)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // Every lane runs the 64 steps - the broadcast of Y8 wants lane k's register whatever lane k does next - and lanes 27 .. 63 add value 0's terms and store
        // nothing. Coefficients 0 and 8 are not in LDS: those lanes read slot 3, which exists, and take the constant or the broadcast instead - chosen with
        // bit masks made outside the loop, not with ?: (the compiler turned that into a branch around the LDS read, with a wait for the read inside it, in
        // every one of the 64 steps: profiles/probe/notes.md).
        const unsigned t = lane < PT_PROBE_VALUES ? lane : 0u;
        const unsigned ci = t / 3u, ch = t - 3u * ci;
        const double* col = fr.lds - lane;  // the wavefront's first column
        const double* ycol = col + (size_t)(ci >= 1u && ci <= 7u ? 2u + ci : 3u) * PT_FRAME_STRIDE;
        const double* vcol = col + (size_t)(PT_L_VALUE + ch) * PT_FRAME_STRIDE;
        const unsigned long long from_lds = ci >= 1u && ci <= 7u ? ~0ull : 0ull, from_lane = ci == 8u ? ~0ull : 0ull;
        const unsigned long long y0_bits = ci == 0u ? (unsigned long long)__double_as_longlong(Y[0]) : 0ull;
        const unsigned long long y8_bits = (unsigned long long)__double_as_longlong(Y[8]);
        double acc = 0.0;
        if (shaded)
#pragma unroll 4  // (unrolled whole, the 128 LDS reads are hoisted in front of the additions and cost the kernel some 150 spilled registers)
            for (unsigned k = 0; k < 64u; k++) {
                const unsigned long long lds_bits = (unsigned long long)__double_as_longlong(ycol[k]);
                const double y = __longlong_as_double((long long)((lds_bits & from_lds) | (pt_probe_lane_u64(y8_bits, k) & from_lane) | y0_bits));
                acc = acc + y * vcol[k];
            }
        if (lane < PT_PROBE_VALUES) {
            if (ab.partial) ab.partial[(size_t)w_again * PT_PROBE_VALUES + lane] = acc;
            else if (ab.sh) ab.sh[(size_t)p_again * PT_PROBE_VALUES + lane] = acc;
        }
        if (lane == 0 && r_again == 0 && ab.valid) ab.valid[p_again] = valid_again ? 1 : 0;
        __builtin_amdgcn_wave_barrier();  // the columns are free for the next item
    }
}

// What pt_shade_launch (pt_shade_frame.h) asks of a pass
struct PtProbePass {
    using Args = PtProbeArgs;
    static PT_HD const PtRenderArgs& render(const PtProbeArgs& a0) { return a0.r; }
    template <int MODE, bool TEX, int PARK>
    static constexpr auto kernel() { return &pt_probe_kernel<MODE, TEX, PARK>; }
};

hipError_t PT_INST_CAT(pt_probe_launch_mode_, PT_INST_MODE)(const PtProbeArgs& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    return pt_shade_launch<PT_INST_MODE, PtProbePass>(a, tex, park, n_cu, stream, grid, launch);
}
