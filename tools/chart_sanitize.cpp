// Stand-alone driver for a sanitizer run of the chart pass's host replay (pt_chart.hip: pt_test_chart_host) on the CPU: `make sanitize-chart` compiles
// pt_chart.hip's host code and this file with -fsanitize=address,undefined, links them with the library's other objects and runs the result. No GPU is touched.
// The case is the watertightness grid of tests/test_chart_contract.py - 8 x 8 quads over the unit square, interior vertices moved by less than a third of a
// cell - at 64 x 64 and 67 x 37, smooth and flat, with triangles that do not take part (a NaN, an inf, a corner beyond 2^24 texels, no area) among them and one
// that reaches far outside the map, so that every clamp of the box is taken. Every output buffer is allocated at its exact size: a write past the map is found.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../include/portrayer_hip.h"

int main() {
    const int cells = 8;
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> off(-0.3 / cells, 0.3 / cells);
    std::vector<double> gu((cells + 1) * (cells + 1)), gv(gu.size());
    for (int j = 0; j <= cells; j++)
        for (int i = 0; i <= cells; i++) {
            const bool inner = i > 0 && i < cells && j > 0 && j < cells;
            gu[j * (cells + 1) + i] = (double)i / cells + (inner ? off(rng) : 0.0);
            gv[j * (cells + 1) + i] = (double)j / cells + (inner ? off(rng) : 0.0);
        }
    std::vector<double> uv;
    auto corner = [&](int i, int j) { uv.push_back(gu[j * (cells + 1) + i]); uv.push_back(gv[j * (cells + 1) + i]); };
    for (int j = 0; j < cells; j++)
        for (int i = 0; i < cells; i++) {
            corner(i, j); corner(i + 1, j); corner(i + 1, j + 1);
            corner(i, j); corner(i + 1, j + 1); corner(i, j + 1);
        }
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double extra[5][6] = {{0.2, nan, 0.8, 0.3, 0.5, 0.9}, {0.2, 0.1, inf, 0.3, 0.5, 0.9}, {0.2, 0.1, 0.8, 0.3, 33554432.0, 0.9}, {0.25, 0.25, 0.5, 0.5, 0.75, 0.75},
                                {-1000.0, -900.0, 1200.0, -800.0, 100.0, 1500.0}};
    for (const auto& e : extra) uv.insert(uv.end(), e, e + 6);
    const uint64_t n_tris = uv.size() / 6;
    std::vector<double> tri_v(9 * n_tris), tri_n(9 * n_tris);
    for (uint64_t k = 0; k < 3 * n_tris; k++) {
        const double u = std::isfinite(uv[2 * k]) ? std::fmax(-4.0, std::fmin(4.0, uv[2 * k])) : 0.3, v = std::isfinite(uv[2 * k + 1]) ? std::fmax(-4.0, std::fmin(4.0, uv[2 * k + 1])) : 0.6;
        tri_v[3 * k] = 2.0 * u - 1.0; tri_v[3 * k + 1] = 2.0 * v - 1.0; tri_v[3 * k + 2] = 0.25 * std::sin(3.0 * u) * std::cos(2.0 * v);
        tri_n[3 * k] = 0.3 * std::cos(3.0 * u); tri_n[3 * k + 1] = 0.2 * std::sin(2.0 * v); tri_n[3 * k + 2] = 1.0;
    }
    const double fwd[12] = {1.1, -0.4, 0.0, 0.3, 0.5, 0.8, -0.2, -1.2, 0.1, 0.3, 2.2, 2.0}, nrm[9] = {0.8, 0.3, -0.1, -0.4, 1.1, 0.2, 0.0, -0.2, 0.45};
    const uint32_t sizes[3][2] = {{64, 64}, {67, 37}, {1, 1}};
    uint64_t covered = 0;
    for (const auto& s : sizes)
        for (int smooth = 0; smooth < 2; smooth++)
            for (uint32_t flags = 0; flags < 2; flags++) {
                const size_t n = (size_t)s[0] * s[1];
                std::vector<double> position(3 * n), normal(3 * n);
                std::vector<int32_t> tri(n);
                std::vector<uint8_t> cov(n);
                const pt_chart_buffers out = {position.data(), normal.data(), tri.data(), cov.data()};
                const int rc = pt_test_chart_host(fwd, nrm, n_tris, tri_v.data(), smooth ? tri_n.data() : nullptr, uv.data(), s[0], s[1], flags, &out);
                if (rc != 0) { std::printf("pt_test_chart_host(%u x %u) returned %d\n", s[0], s[1], rc); return 1; }
                for (size_t q = 0; q < n; q++) {
                    if (!cov[q] || tri[q] < 0 || (uint64_t)tri[q] >= n_tris) { std::printf("%u x %u: texel %zu is not covered\n", s[0], s[1], q); return 1; }
                    covered++;
                }
                const pt_chart_buffers only = {nullptr, nullptr, tri.data(), nullptr};
                if (pt_test_chart_host(fwd, nrm, n_tris, tri_v.data(), nullptr, uv.data(), s[0], s[1], flags, &only) != 0) return 1;
            }
    const pt_chart_buffers none = {nullptr, nullptr, nullptr, nullptr};
    if (pt_test_chart_host(fwd, nrm, n_tris, tri_v.data(), nullptr, uv.data(), 8, 8, 0, &none) == 0) { std::printf("no output buffer was not refused\n"); return 1; }
    std::printf("chart_sanitize: %llu triangles, %llu texels covered, clean\n", (unsigned long long)n_tris, (unsigned long long)covered);
    return 0;
}
