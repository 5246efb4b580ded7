// Stand-alone driver for a sanitizer run of the slab-test hook (pt_api.hip: pt_test_raypk) on the CPU: `make sanitize-raypk` compiles pt_api.hip's host
// code and this file with -fsanitize=address,undefined, links them with the library's other objects and runs the result. No GPU is touched.
// Rays and boxes of every kind tests/test_raypk_conservative.py draws: ordinary ones, zero / denormal / huge direction components, boxes at the limit
// of +-1e18, a face through the origin, infinite and tiny ranges; every body of the constants.
#include <cmath>
#include <cstdint>
#include <cstdio>
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
    return 0;
}
