// Stand-alone driver for a sanitizer run of the host-side hooks of pt_api.hip (pt_test_raypk, the beam tests, pt_test_dark_light, pt_test_launch_plan) on the CPU: `make sanitize-raypk` compiles pt_api.hip's host
// code and this file with -fsanitize=address,undefined, links them with the library's other objects and runs the result. No GPU is touched.
// Rays and boxes of every kind tests/test_raypk_conservative.py draws: ordinary ones, zero / denormal / huge direction components, boxes at the limit
// of +-1e18, a face through the origin, infinite and tiny ranges; every body of the constants.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../include/portrayer_hip.h"

int main() {
    const uint64_t n = 200000;
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> u(-1.0, 1.0), e(-3.0, 6.0);
    const double special[] = {0.0, -0.0, 5e-324, -1e-310, 1e-40, -1e-45, 1e-19, -1.1e-18, 1e-18, 3e38, -1e300, 1.0, -1.0};
    std::vector<double> o(3 * n), d(3 * n), tm(n);
    std::vector<float> lo(3 * n), hi(3 * n), tn(n), tf(n);
    std::vector<int32_t> verdict(n);
    for (uint64_t i = 0; i < n; i++) {
        for (int k = 0; k < 3; k++) {
            o[3 * i + k] = u(rng) * std::pow(10.0, e(rng));
            d[3 * i + k] = (rng() % 5 == 0) ? special[rng() % 13] : u(rng) * std::pow(10.0, 0.5 * e(rng));
            const double c = (rng() % 7 == 0) ? u(rng) * 1e18 : o[3 * i + k] + u(rng) * std::pow(10.0, e(rng));
            const double h = std::fabs(c) * std::pow(10.0, e(rng) - 6.0);
            lo[3 * i + k] = (float)std::fmax(c - h, -1e18);
            hi[3 * i + k] = (float)std::fmin(std::fmax(c + h, (double)lo[3 * i + k]), 1e18);
            if (rng() % 11 == 0) { o[3 * i + k] = (double)(float)o[3 * i + k]; lo[3 * i + k] = (float)o[3 * i + k]; if (hi[3 * i + k] < lo[3 * i + k]) hi[3 * i + k] = lo[3 * i + k]; }
        }
        tm[i] = (rng() % 3 == 0) ? std::numeric_limits<double>::infinity() : std::pow(10.0, e(rng)) * (rng() % 9 == 0 ? 1e-30 : 1.0);
    }
    uint64_t accepted = 0;
    for (int body = 0; body < 3; body++) {
        const int rc = pt_test_raypk(n, body, o.data(), d.data(), tm.data(), lo.data(), hi.data(), verdict.data(), tn.data(), tf.data());
        if (rc != 0) { std::printf("pt_test_raypk(body %d) returned %d\n", body, rc); return 1; }
        for (uint64_t i = 0; i < n; i++) accepted += (uint64_t)(verdict[i] & 1);
    }
    if (pt_test_raypk(1, 3, o.data(), d.data(), tm.data(), lo.data(), hi.data(), verdict.data(), tn.data(), tf.data()) == 0) { std::printf("body 3 was not refused\n"); return 1; }
    if (pt_test_raypk(0, 0, o.data(), d.data(), tm.data(), lo.data(), hi.data(), verdict.data(), tn.data(), tf.data()) != 0) { std::printf("n = 0 failed\n"); return 1; }
    std::printf("raypk_sanitize ok: %llu pairs x 3 bodies, %llu accepted\n", (unsigned long long)n, (unsigned long long)accepted);

    // The pixel lists' beam test (pt_test_pixel_beam) on the same boxes: cameras at random and degenerate ones (zero and non-finite fields, a zero-sized image),
    // pixels inside and far outside the image, jitters at the ends of [0, 1).
    std::vector<double> cams(19 * n), jit(2 * n), rays(6 * n);
    std::vector<uint32_t> pix(2 * n);
    std::vector<int32_t> accept(n), walk(n);
    std::vector<float> bound(n);
    const double odd[] = {0.0, -0.0, 1e-310, 1e300, -1e300, std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN()};
    for (uint64_t i = 0; i < n; i++) {
        double* c = &cams[19 * i];
        for (int k = 0; k < 15; k++) c[k] = u(rng) * (k < 3 ? std::pow(10.0, e(rng)) : 1.0);
        for (int k = 0; k < 3; k++) c[3 + 4 * k + 3] = c[k];
        c[15] = 0.05 + std::fabs(u(rng)) * 2.0; c[17] = (double)(1 + rng() % 2000); c[18] = (double)(1 + rng() % 1200); c[16] = c[17] / c[18];
        if (rng() % 9 == 0) c[rng() % 19] = odd[rng() % 7];
        pix[2 * i] = (rng() % 13 == 0) ? (uint32_t)rng() : (uint32_t)(rng() % 2000);
        pix[2 * i + 1] = (rng() % 13 == 0) ? (uint32_t)rng() : (uint32_t)(rng() % 1200);
        for (int k = 0; k < 2; k++) jit[2 * i + k] = (rng() % 5 == 0) ? 0.0 : ((rng() % 5 == 0) ? 1.0 - 0x1p-53 : 0.5 + 0.5 * u(rng) * (1.0 - 0x1p-53));
    }
    int rc = pt_test_pixel_beam(n, cams.data(), pix.data(), jit.data(), lo.data(), hi.data(), accept.data(), bound.data(), walk.data(), rays.data());
    if (rc != 0) { std::printf("pt_test_pixel_beam returned %d\n", rc); return 1; }
    uint64_t listed = 0, walked = 0;
    for (uint64_t i = 0; i < n; i++) { listed += (uint64_t)accept[i]; walked += walk[i] != 0; if (accept[i] && !(bound[i] >= 0.0f)) { std::printf("case %llu: a bound that is no number\n", (unsigned long long)i); return 1; } }
    if (pt_test_pixel_beam(n, cams.data(), pix.data(), jit.data(), lo.data(), hi.data(), accept.data(), bound.data(), walk.data(), nullptr) != 0) { std::printf("rays = NULL failed\n"); return 1; }
    if (pt_test_pixel_beam(1, nullptr, pix.data(), jit.data(), lo.data(), hi.data(), accept.data(), bound.data(), walk.data(), nullptr) == 0) { std::printf("cameras = NULL was not refused\n"); return 1; }
    if (pt_test_pixel_beam(0, cams.data(), pix.data(), jit.data(), lo.data(), hi.data(), accept.data(), bound.data(), walk.data(), nullptr) != 0) { std::printf("n = 0 failed\n"); return 1; }
    std::printf("pixel beam ok: %llu cases, %llu listed, %llu accepted by the walk\n", (unsigned long long)n, (unsigned long long)listed, (unsigned long long)walked);

    // The same test with a rectangle per case (pt_test_rect_beam), on the same cameras - the degenerate ones included - and boxes: the list kernel's 8 x 8 tile, rows and
    // columns, zero-sized rectangles (one sample position, a line of them), huge ones; the sample at a corner of its rectangle or inside. A rectangle of 1 x 1 must repeat
    // the pixel's verdict and bound.
    std::vector<uint32_t> rect(4 * n);
    std::vector<double> off(2 * n);
    std::vector<int32_t> accept_r(n), walk_r(n);
    std::vector<float> bound_r(n);
    const uint32_t sizes[] = {8, 1, 0, 8, 1, 0, 64, 0xFFFFFFFFu};
    for (uint64_t i = 0; i < n; i++) {
        rect[4 * i] = pix[2 * i]; rect[4 * i + 1] = pix[2 * i + 1];
        const bool as_pixel = i % 4 == 0;
        rect[4 * i + 2] = as_pixel ? 1u : sizes[rng() % 8]; rect[4 * i + 3] = as_pixel ? 1u : sizes[rng() % 8];
        for (int k = 0; k < 2; k++) off[2 * i + k] = as_pixel ? jit[2 * i + k] : (double)rect[4 * i + 2 + k] * ((rng() % 3 == 0) ? 0.0 : ((rng() % 3 == 0) ? 1.0 : 0.5 + 0.5 * u(rng)));
    }
    rc = pt_test_rect_beam(n, cams.data(), rect.data(), off.data(), lo.data(), hi.data(), accept_r.data(), bound_r.data(), walk_r.data(), rays.data());
    if (rc != 0) { std::printf("pt_test_rect_beam returned %d\n", rc); return 1; }
    uint64_t listed_r = 0;
    for (uint64_t i = 0; i < n; i++) {
        listed_r += (uint64_t)accept_r[i];
        if (accept_r[i] && !(bound_r[i] >= 0.0f)) { std::printf("rectangle case %llu: a bound that is no number\n", (unsigned long long)i); return 1; }
        if (i % 4 == 0 && (accept_r[i] != accept[i] || bound_r[i] != bound[i] || walk_r[i] != walk[i])) { std::printf("rectangle case %llu: 1 x 1 differs from the pixel\n", (unsigned long long)i); return 1; }
    }
    if (pt_test_rect_beam(n, cams.data(), rect.data(), off.data(), lo.data(), hi.data(), accept_r.data(), bound_r.data(), walk_r.data(), nullptr) != 0) { std::printf("rectangles, rays = NULL failed\n"); return 1; }
    if (pt_test_rect_beam(1, cams.data(), nullptr, off.data(), lo.data(), hi.data(), accept_r.data(), bound_r.data(), walk_r.data(), nullptr) == 0) { std::printf("rects = NULL was not refused\n"); return 1; }
    if (pt_test_rect_beam(0, cams.data(), rect.data(), off.data(), lo.data(), hi.data(), accept_r.data(), bound_r.data(), walk_r.data(), nullptr) != 0) { std::printf("rectangles, n = 0 failed\n"); return 1; }
    std::printf("rectangle beam ok: %llu cases, %llu listed\n", (unsigned long long)n, (unsigned long long)listed_r);

    // The dark-light test (pt_test_dark_light): every type tag, ordinary nodes (a scaled identity at a random centre, the light somewhere in or around it) and degenerate
    // records - zero radius (a zero matrix), NaN and infinite entries, matrices that are no pair, P and L coincident, NaN / infinite / huge P and L, area vectors zero, tiny and NaN.
    const uint64_t m = 50000;
    std::vector<double> fwd(12 * m), inv(12 * m), P(3 * m), L(3 * m), area(6 * m);
    std::vector<int32_t> flagged(m), guard(m), exact(m);
    uint64_t n_flagged = 0, n_guard = 0;
    for (int type = 0; type < 8; type++) {
        for (uint64_t i = 0; i < m; i++) {
            const double s = std::pow(10.0, e(rng));
            for (int k = 0; k < 12; k++) fwd[12 * i + k] = inv[12 * i + k] = 0.0;
            for (int k = 0; k < 3; k++) {
                const double c = u(rng) * std::pow(10.0, e(rng));
                fwd[12 * i + 5 * k] = s; fwd[12 * i + 4 * k + 3] = c;
                inv[12 * i + 5 * k] = 1.0 / s; inv[12 * i + 4 * k + 3] = -c / s;
                L[3 * i + k] = c + u(rng) * s * 0.7;
                P[3 * i + k] = (rng() % 4 == 0) ? L[3 * i + k] : L[3 * i + k] + u(rng) * std::pow(10.0, e(rng));
            }
            for (int k = 0; k < 6; k++) area[6 * i + k] = (rng() % 3 == 0) ? u(rng) * std::pow(10.0, -50.0 * std::fabs(u(rng))) : 0.0;
            switch (rng() % 8) {
                case 0: for (int k = 0; k < 12; k++) fwd[12 * i + k] = inv[12 * i + k] = 0.0; break;  // zero radius
                case 1: fwd[12 * i + rng() % 12] = odd[rng() % 7]; break;
                case 2: inv[12 * i + rng() % 12] = odd[rng() % 7]; break;
                case 3: L[3 * i + rng() % 3] = odd[rng() % 7]; break;
                case 4: P[3 * i + rng() % 3] = odd[rng() % 7]; break;
                case 5: area[6 * i + rng() % 6] = odd[rng() % 7]; break;
                default: break;
            }
        }
        rc = pt_test_dark_light(m, type, fwd.data(), inv.data(), P.data(), L.data(), (type & 1) ? nullptr : area.data(), flagged.data(), guard.data(), exact.data());
        if (rc != 0) { std::printf("pt_test_dark_light(type %d) returned %d\n", type, rc); return 1; }
        for (uint64_t i = 0; i < m; i++) {
            n_flagged += (uint64_t)flagged[i]; n_guard += (uint64_t)guard[i];
            if (guard[i] && !flagged[i]) { std::printf("type %d case %llu: the guard without the flag\n", type, (unsigned long long)i); return 1; }
            if (flagged[i] && type != 0 && type != 5) { std::printf("type %d case %llu: flagged without a ball\n", type, (unsigned long long)i); return 1; }
            if (guard[i] && P[3 * i] == L[3 * i] && P[3 * i + 1] == L[3 * i + 1] && P[3 * i + 2] == L[3 * i + 2]) { std::printf("type %d case %llu: P == L through the guard\n", type, (unsigned long long)i); return 1; }
            if (guard[i] && !exact[i]) { std::printf("type %d case %llu: skipped without an exact hit\n", type, (unsigned long long)i); return 1; }
        }
    }
    if (pt_test_dark_light(1, 8, fwd.data(), inv.data(), P.data(), L.data(), nullptr, flagged.data(), guard.data(), exact.data()) == 0) { std::printf("type 8 was not refused\n"); return 1; }
    if (pt_test_dark_light(1, 0, fwd.data(), inv.data(), P.data(), nullptr, nullptr, flagged.data(), guard.data(), exact.data()) == 0) { std::printf("L = NULL was not refused\n"); return 1; }
    if (pt_test_dark_light(0, 0, fwd.data(), inv.data(), P.data(), L.data(), nullptr, flagged.data(), guard.data(), exact.data()) != 0) { std::printf("dark light, n = 0 failed\n"); return 1; }
    if (n_flagged == 0 || n_guard == 0) { std::printf("dark light: nothing flagged\n"); return 1; }
    std::printf("dark light ok: %llu cases x 8 types, %llu flagged, %llu through the guard\n", (unsigned long long)m, (unsigned long long)n_flagged, (unsigned long long)n_guard);

    // The launch planner (pt_test_launch_plan): every mode, plain and counting, with sizes at the ends of their ranges - no nodes, no lights, no slots, the most of each, a
    // grid of one block and a huge one - under the switches at hostile values; a malformed switch must be refused with its words cut to the caller's buffer.
    const char* const envs[][2] = {{"PORTRAYER_OCC_SEED", "18446744073709551615"}, {"PORTRAYER_OCC_SEED", "all:0"}, {"PORTRAYER_PIXEL_LIST_CAP", "0"}, {"PORTRAYER_PIXEL_LIST_PENDING", "1"},
                                   {"PORTRAYER_FINE_QUEUES", "2147483647"}, {"PORTRAYER_BATCH_MAX", "-2147483648"}, {"PORTRAYER_ITEM_STRIDE", "golden"}, {"PORTRAYER_ITEM_STRIDE", "-7"},
                                   {"PORTRAYER_LDS_STACK", "0"}, {"PORTRAYER_LDS_BUDGET_KB", "999"}};
    const uint32_t ends[] = {0u, 1u, 64u, 65536u, 65537u, 0xFFFFFFC0u};
    uint64_t plans = 0, lists = 0;
    for (int env = -1; env < 10; env++) {
        if (env >= 0) setenv(envs[env][0], envs[env][1], 1);
        for (int k = 0; k < 54; k++) {
            pt_launch_query q = {};
            q.traits.traverse = 1 + k % 3; q.traits.n_nodes = ends[(k / 5) % 6]; q.traits.n_lights = ends[(k / 2) % 4]; q.traits.reflective = k % 5 == 0; q.traits.reflective_opaque = k % 2;
            q.mode = k % 10 == 0 ? -1 : 1 + k % 9; q.textured = k % 4 == 0; q.stats = k % 3 == 0;
            q.n_nodes = q.traits.n_nodes; q.n_lights = q.traits.n_lights; q.stack_cap = (int32_t)(1 + ends[k % 5] % 4096u);
            q.n_slots = ends[(k / 3) % 6]; q.n_chunks = 1 + k % 13; q.k_log2 = 3; q.c_log2 = 2 + k % 2; q.n_items = ends[(k / 3) % 6] / 64u * 64u;
            q.tiles_x = ends[k % 6]; q.tile_ranks = ends[(k / 6) % 3]; q.grid = (k % 7 == 0) ? 1u : ((k % 7 == 1) ? 0xFFFFFFu : 768u);
            uint64_t words[PT_PLAN_WORDS];
            char why[16];
            rc = pt_test_launch_plan(&q, words, why, sizeof why);
            if (rc != 0 && !(env == 1 && q.n_nodes == 0)) { std::printf("pt_test_launch_plan (switch %d, case %d) returned %d: %s\n", env, k, rc, why); return 1; }
            if (rc == 0) { plans++; lists += (words[PT_PLAN_HAS] & PT_PLAN_HAS_PIXEL_LISTS) != 0; }
            if (rc == 0 && words[PT_PLAN_MISC_BYTES] != words[PT_PLAN_OCC_OFF] + words[PT_PLAN_OCC_BYTES]) { std::printf("switch %d, case %d: misc does not end with the occluder table\n", env, k); return 1; }
        }
        if (env >= 0) unsetenv(envs[env][0]);
    }
    pt_launch_query q = {};
    q.traits.traverse = 1; q.traits.n_nodes = q.n_nodes = 5; q.traits.n_lights = q.n_lights = 2; q.traits.reflective_opaque = 1; q.mode = -1; q.stack_cap = 16;
    q.n_slots = 256; q.n_items = 16384; q.n_chunks = 8; q.k_log2 = q.c_log2 = 3; q.tiles_x = 2; q.tile_ranks = 1; q.grid = 768;
    uint64_t words[PT_PLAN_WORDS];
    char why[24];
    setenv("PORTRAYER_PIXEL_LIST_CAP", "a value far longer than the buffer its refusal is copied to", 1);
    if (pt_test_launch_plan(&q, words, why, sizeof why) != -1 || std::strlen(why) != sizeof why - 1) { std::printf("a malformed list cap was not refused\n"); return 1; }
    if (pt_test_launch_plan(&q, words, nullptr, 0) != -1 || pt_test_launch_plan(&q, nullptr, why, sizeof why) != -1 || pt_test_launch_plan(nullptr, words, why, sizeof why) != -1) { std::printf("NULL arguments\n"); return 1; }
    unsetenv("PORTRAYER_PIXEL_LIST_CAP");
    if (pt_test_launch_plan(&q, words, why, sizeof why) != 0 || !(words[PT_PLAN_HAS] & PT_PLAN_HAS_QUEUE)) { std::printf("the five-node launch has no queue\n"); return 1; }
    if (lists == 0) { std::printf("launch plan: no case had lists\n"); return 1; }
    std::printf("launch plan ok: %llu plans, %llu with lists\n", (unsigned long long)plans, (unsigned long long)lists);
    return 0;
}
