// The denoiser's kernels (pt_film_denoise*, include/portrayer_hip.h) and its host replay. The arithmetic is pt_denoise.h's and nothing else: a
// SEED kernel makes level 0's (c, v) out of the film's state, one FILTER kernel per level reads level l and writes level l + 1, a FINISH kernel writes the
// caller's buffers. The filter exists in two forms that compute the same bits (the result does not depend on the schedule):
//   direct  one thread per pixel, its 25 taps from global memory;
//   tiled   a 256-thread block owns 16 x 16 pixels of ONE residue class modulo the step s (x = rx + s i, y = ry + s j): in class space every level is a plain
//           5 x 5 stencil with a halo of 2, so the block stages 20 x 20 records into LDS - every component an f64 array of its own, consecutive lanes on
//           consecutive banks - and filters from there.
// No kernel waits on another block; every loop is bounded by a constant (25 taps, the staging rounds of a block).
#include <hip/hip_runtime.h>

#include "../../include/portrayer_hip.h"
#include "pt_denoise.h"
#include "pt_denoise_pixel.h"

// One thread per pixel of the image. Pixels without samples are neither centres nor taps: their record is never read, so none is written.
__global__ void __launch_bounds__(256) pt_denoise_seed_kernel(uint32_t n_pixels, const double* __restrict__ total, const double* __restrict__ partial, const uint32_t* __restrict__ count,
                                                             const double* __restrict__ q2, double* __restrict__ work) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    const uint32_t n = count[p];
    if (n == 0u) return;
    const double *t = total + 3 * (size_t)p, *q = partial + 3 * (size_t)p;
    const PtVec3 tot = pt_v3(t[0], t[1], t[2]), par = pt_v3(q[0], q[1], q[2]);
    const PtVec3 c = pt_film_sum(tot, par, n) / (double)n;  // resolve's `linear`
    const double err = q2 && n >= 2u ? pt_film_error_of(tot, par, q2[p], n) : 0.0;
    double* o = work + 4 * (size_t)p;
    o[0] = c.x; o[1] = c.y; o[2] = c.z;
    o[3] = pt_denoise_seed_variance(c, n, q2 != nullptr, err);
}

// The record of pixel `at` (inside the film, count > 0) from global memory.
static __device__ PtDenoisePix pt_denoise_load(const PtDenoiseLevelArgs& a, size_t at, bool want_n, bool want_pos) {
    PtDenoisePix r;
    const double* cv = a.in + 4 * at;
    r.c = pt_v3(cv[0], cv[1], cv[2]);
    r.v = cv[3];
    r.node = a.node[at];
    r.n = r.pos = pt_v3(0.0, 0.0, 0.0);
    if (want_n) { const double* n = a.normal + 3 * at; r.n = pt_v3(n[0], n[1], n[2]); }
    if (want_pos) { const double* s = a.position + 3 * at; r.pos = pt_v3(s[0], s[1], s[2]); }
    return r;
}

// (a) direct: one thread per pixel of the image.
__global__ void __launch_bounds__(256) pt_denoise_direct_kernel(PtDenoiseLevelArgs a) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.width * a.height) return;
    if (a.count[p] == 0u) return;
    const bool want_n = a.k.normal_pow >= 0 || a.k.use_plane, want_pos = a.k.use_plane != 0u;
    const int x = (int)(p % a.width), y = (int)(p / a.width), s = (int)a.step;
    const PtDenoisePix P = pt_denoise_load(a, p, want_n, want_pos);
    PtDenoiseAcc acc = pt_denoise_acc_zero();
    for (int j = -2; j <= 2; j++) {
        const int qy = y + s * j;
        if (qy < 0 || qy >= (int)a.height) continue;
        for (int i = -2; i <= 2; i++) {
            const int qx = x + s * i;
            if (qx < 0 || qx >= (int)a.width) continue;
            const size_t at = (size_t)qy * a.width + (size_t)qx;
            if (a.count[at] == 0u) continue;
            const PtDenoisePix Q = pt_denoise_load(a, at, want_n, want_pos);
            pt_denoise_accumulate(acc, Q.c, Q.v, pt_denoise_weight(a.k, i, j, P, Q));
        }
    }
    PtVec3 c;
    double v;
    pt_denoise_level_out(acc, P.c, P.v, &c, &v);
    double* o = a.out + 4 * (size_t)p;
    o[0] = c.x; o[1] = c.y; o[2] = c.z; o[3] = v;
}

// (b) tiled. blockIdx.z names the residue class (rx, ry) = (z % s, z / s); in class space the image is cw x ch pixels, blockIdx.x / .y the 16 x 16 tile
// of it. Cell (lx, ly) of the staged square is class pixel (16 bx - 2 + lx, 16 by - 2 + ly); `valid` = inside the film with count > 0.
// The lanes of a half-wavefront sit on rows r and r + 4 of the tile: 4 rows of 20 f64 are 80 f64 = 16 modulo 32, so the two groups of 16 lanes read the two
// halves of the 64 banks an 8-byte LDS read spans and no two lanes of a half meet on one.
__global__ void __launch_bounds__(256) pt_denoise_tiled_kernel(PtDenoiseLevelArgs a) {
    __shared__ double s_c[3][PT_DN_CELLS], s_v[PT_DN_CELLS], s_n[3][PT_DN_CELLS], s_pos[3][PT_DN_CELLS];
    __shared__ int32_t s_node[PT_DN_CELLS];
    __shared__ uint32_t s_valid[PT_DN_CELLS];
    static_assert(sizeof s_c + sizeof s_v + sizeof s_n + sizeof s_pos + sizeof s_node + sizeof s_valid == PT_DN_LDS_BYTES, "DESIGN 4.14 states the block's LDS");
    const bool want_n = a.k.normal_pow >= 0 || a.k.use_plane, want_pos = a.k.use_plane != 0u;
    const int s = (int)a.step;
    const int rx = (int)(blockIdx.z % a.step), ry = (int)(blockIdx.z / a.step);
    const int cx0 = (int)blockIdx.x * PT_DN_TILE - PT_DN_HALO, cy0 = (int)blockIdx.y * PT_DN_TILE - PT_DN_HALO;
    // stage: cell = t, t + 256 (two rounds cover the 400 cells)
    for (int cell = (int)threadIdx.x; cell < PT_DN_CELLS; cell += 256) {
        const int lx = cell % PT_DN_SIDE, ly = cell / PT_DN_SIDE;
        const int cx = cx0 + lx, cy = cy0 + ly;
        const long gx = (long)rx + (long)s * cx, gy = (long)ry + (long)s * cy;
        bool valid = cx >= 0 && cy >= 0 && gx < (long)a.width && gy < (long)a.height;
        size_t at = 0;
        if (valid) {
            at = (size_t)gy * a.width + (size_t)gx;
            valid = a.count[at] != 0u;
        }
        PtDenoisePix r;
        r.c = r.n = r.pos = pt_v3(0.0, 0.0, 0.0);
        r.v = 0.0;
        r.node = -1;
        if (valid) r = pt_denoise_load(a, at, want_n, want_pos);
        s_c[0][cell] = r.c.x; s_c[1][cell] = r.c.y; s_c[2][cell] = r.c.z;
        s_v[cell] = r.v;
        if (want_n) { s_n[0][cell] = r.n.x; s_n[1][cell] = r.n.y; s_n[2][cell] = r.n.z; }
        if (want_pos) { s_pos[0][cell] = r.pos.x; s_pos[1][cell] = r.pos.y; s_pos[2][cell] = r.pos.z; }
        s_node[cell] = r.node;
        s_valid[cell] = valid ? 1u : 0u;
    }
    __syncthreads();
    const int t = (int)threadIdx.x;
    const int tx = t & 15, half = t >> 5, sub = (t >> 4) & 1;
    const int ty = (half & 3) + 4 * sub + 8 * (half >> 2);
    const int centre = (ty + PT_DN_HALO) * PT_DN_SIDE + tx + PT_DN_HALO;
    if (!s_valid[centre]) return;  // outside the film, or a pixel without samples (no barrier follows)
    auto cell_pix = [&](int cell) {
        PtDenoisePix r;
        r.c = pt_v3(s_c[0][cell], s_c[1][cell], s_c[2][cell]);
        r.v = s_v[cell];
        r.node = s_node[cell];
        r.n = r.pos = pt_v3(0.0, 0.0, 0.0);
        if (want_n) r.n = pt_v3(s_n[0][cell], s_n[1][cell], s_n[2][cell]);
        if (want_pos) r.pos = pt_v3(s_pos[0][cell], s_pos[1][cell], s_pos[2][cell]);
        return r;
    };
    const PtDenoisePix P = cell_pix(centre);
    PtDenoiseAcc acc = pt_denoise_acc_zero();
    for (int j = -2; j <= 2; j++)
        for (int i = -2; i <= 2; i++) {
            const int cell = centre + j * PT_DN_SIDE + i;  // (inside the staged square: the halo is 2)
            if (!s_valid[cell]) continue;
            const PtDenoisePix Q = cell_pix(cell);
            pt_denoise_accumulate(acc, Q.c, Q.v, pt_denoise_weight(a.k, i, j, P, Q));
        }
    PtVec3 c;
    double v;
    pt_denoise_level_out(acc, P.c, P.v, &c, &v);
    const size_t gx = (size_t)rx + (size_t)s * (size_t)(cx0 + PT_DN_HALO + tx), gy = (size_t)ry + (size_t)s * (size_t)(cy0 + PT_DN_HALO + ty);  // (valid: inside the film)
    double* o = a.out + 4 * (gy * a.width + gx);
    o[0] = c.x; o[1] = c.y; o[2] = c.z; o[3] = v;
}

// One thread per pixel of the image: the last level's record out, rgb by resolve's finishing (pt_film_resolve_kernel).
__global__ void __launch_bounds__(256) pt_denoise_finish_kernel(uint32_t n_pixels, const double* __restrict__ work, const uint32_t* __restrict__ count, uint8_t* __restrict__ rgb,
                                                               double* __restrict__ linear, double* __restrict__ variance) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    if (count[p] == 0u) return;
    const double* cv = work + 4 * (size_t)p;
    pt_denoise_finish_pixel(p, pt_v3(cv[0], cv[1], cv[2]), cv + 3, rgb, linear, variance);
}

hipError_t pt_denoise_seed_launch(uint32_t width, uint32_t height, const double* total, const double* partial, const uint32_t* count, const double* q, double* work, hipStream_t stream) {
    const uint32_t n = width * height;  // (pt_film_create refuses films of 2^31 pixels or more)
    hipLaunchKernelGGL(pt_denoise_seed_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, n, total, partial, count, q, work);
    return hipGetLastError();
}

hipError_t pt_denoise_level_launch(const PtDenoiseLevelArgs& a, bool tiled, hipStream_t stream) {
    if (!tiled) {
        const uint32_t n = a.width * a.height;
        hipLaunchKernelGGL(pt_denoise_direct_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, a);
        return hipGetLastError();
    }
    // class space: the largest class is ceil(width / s) x ceil(height / s); smaller classes leave cells of their last tiles invalid. s <= 128: s * s <= 16384 classes.
    const uint32_t s = a.step;
    const uint32_t cw = (a.width + s - 1u) / s, ch = (a.height + s - 1u) / s;
    const uint32_t classes_y = s < a.height ? s : a.height;  // (rows of classes past the image hold no pixel; a class column past it finds every cell invalid)
    const dim3 grid((cw + PT_DN_TILE - 1u) / PT_DN_TILE, (ch + PT_DN_TILE - 1u) / PT_DN_TILE, s * classes_y);
    hipLaunchKernelGGL(pt_denoise_tiled_kernel, grid, dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t pt_denoise_finish_launch(uint32_t width, uint32_t height, const double* work, const uint32_t* count, uint8_t* rgb, double* linear, double* variance, hipStream_t stream) {
    const uint32_t n = width * height;
    hipLaunchKernelGGL(pt_denoise_finish_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, n, work, count, rgb, linear, variance);
    return hipGetLastError();
}

// What every entry point refuses of the parameters and the guides, in the header's order. NULL = fine, else the message.
const char* pt_denoise_check(const pt_denoise_params* p, const pt_denoise_guides* g) {
    if (!p || !g) return "NULL params or guides";
    if (p->iterations < 1 || p->iterations > PT_DENOISE_MAX_ITERATIONS) return "iterations is 1 .. 8";
    if (p->flags & ~(uint32_t)PT_DENOISE_SAME_NODE) return "unknown flags";
    if (!(p->sigma_color >= 0.0) || !(p->sigma_color <= 1.7976931348623157e308)) return "sigma_color must be finite and >= 0";
    if (!(p->sigma_plane >= 0.0) || !(p->sigma_plane <= 1.7976931348623157e308)) return "sigma_plane must be finite and >= 0";
    if (p->normal_power_log2 < -1 || p->normal_power_log2 > PT_DENOISE_MAX_NORMAL_POWER_LOG2) return "normal_power_log2 is -1 .. 7";
    if (!g->node) return "the node guide is required";
    if (!g->normal && (p->normal_power_log2 >= 0 || p->sigma_plane > 0.0)) return "the normal guide is required with a normal or a plane weight";
    if (!g->position && p->sigma_plane > 0.0) return "the position guide is required with a plane weight";
    return nullptr;
}

// Host-side replay (no GPU, no context): the plain loop over pt_denoise.h's functions, level after level, from a level-0 input the caller supplies.
extern "C" int pt_test_denoise_host(uint32_t width, uint32_t height, const pt_denoise_params* params, const double* linear, const double* variance, const uint32_t* counts,
                                    const pt_denoise_guides* guides, double* out_linear, double* out_variance) {
    if (pt_denoise_check(params, guides) || !linear || !counts || (!out_linear && !out_variance) || width == 0 || height == 0 || (uint64_t)width * height >= 0x80000000ull)
        return PT_ERR_ARGUMENT;
    if (!variance && params->sigma_color > 0.0) return PT_ERR_ARGUMENT;  // (a film without moments: v = 0, accepted without a colour weight only)
    const PtDenoiseConst k = pt_denoise_const(*params);
    const bool want_n = k.normal_pow >= 0 || k.use_plane, want_pos = k.use_plane != 0u;
    const size_t n = (size_t)width * height;
    double* work[2] = {new double[4 * n], new double[4 * n]};
    for (size_t p = 0; p < n; p++) {
        double* o = work[0] + 4 * p;
        o[0] = linear[3 * p]; o[1] = linear[3 * p + 1]; o[2] = linear[3 * p + 2];
        o[3] = variance ? variance[p] : 0.0;
    }
    auto pix = [&](const double* in, size_t at) {
        PtDenoisePix r;
        r.c = pt_v3(in[4 * at], in[4 * at + 1], in[4 * at + 2]);
        r.v = in[4 * at + 3];
        r.node = guides->node[at];
        r.n = r.pos = pt_v3(0.0, 0.0, 0.0);
        if (want_n) r.n = pt_v3(guides->normal[3 * at], guides->normal[3 * at + 1], guides->normal[3 * at + 2]);
        if (want_pos) r.pos = pt_v3(guides->position[3 * at], guides->position[3 * at + 1], guides->position[3 * at + 2]);
        return r;
    };
    int cur = 0;
    for (int l = 0; l < params->iterations; l++, cur ^= 1) {
        const double* in = work[cur];
        double* out = work[cur ^ 1];
        const long s = 1L << l;
        for (long y = 0; y < (long)height; y++)
            for (long x = 0; x < (long)width; x++) {
                const size_t p = (size_t)y * width + (size_t)x;
                if (counts[p] == 0u) continue;
                const PtDenoisePix P = pix(in, p);
                PtDenoiseAcc acc = pt_denoise_acc_zero();
                for (int j = -2; j <= 2; j++)
                    for (int i = -2; i <= 2; i++) {
                        const long qx = x + s * i, qy = y + s * j;
                        if (qx < 0 || qy < 0 || qx >= (long)width || qy >= (long)height) continue;
                        const size_t at = (size_t)qy * width + (size_t)qx;
                        if (counts[at] == 0u) continue;
                        const PtDenoisePix Q = pix(in, at);
                        pt_denoise_accumulate(acc, Q.c, Q.v, pt_denoise_weight(k, i, j, P, Q));
                    }
                PtVec3 c;
                double v;
                pt_denoise_level_out(acc, P.c, P.v, &c, &v);
                out[4 * p] = c.x; out[4 * p + 1] = c.y; out[4 * p + 2] = c.z; out[4 * p + 3] = v;
            }
    }
    for (size_t p = 0; p < n; p++) {
        if (counts[p] == 0u) continue;  // left untouched, as in resolve
        const double* cv = work[cur] + 4 * p;
        if (out_linear) { out_linear[3 * p] = cv[0]; out_linear[3 * p + 1] = cv[1]; out_linear[3 * p + 2] = cv[2]; }
        if (out_variance) out_variance[p] = cv[3];
    }
    delete[] work[0];
    delete[] work[1];
    return PT_OK;
}
