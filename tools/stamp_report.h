// tools/stamp_report.h -- the start / end stamps that the convolution kernels write per workgroup under their probe-only ABL bit
// (device-wide 100 MHz counter: 10 ns ticks; [2 * workgroup] start, [2 * workgroup + 1] end), printed the way `wino_probe split` prints
// them, and the ends grouped by blockIdx.x < CUs (the first workgroup a CU receives) and >= CUs (the second: tools/census_probe.hip).
#pragma once
#include <algorithm>
#include <cstdio>
#include <vector>

static inline void stamp_report(const char *what, const std::vector<long long> &ht, int grid, int cus) {
    long long t0 = ht[0];
    for (int i = 0; i < grid; ++i) t0 = std::min(t0, ht[2 * i]);
    std::vector<double> st, en, lo, hi, lone;
    for (int i = 0; i < grid; ++i) {
        const double e = (ht[2 * i + 1] - t0) * 0.01;
        st.push_back((ht[2 * i] - t0) * 0.01), en.push_back(e);
        // a workgroup below CUs whose partner index does not exist has its CU to itself (as far as placement follows the index)
        if (i >= cus) hi.push_back(e);
        else if (i + cus < grid) lo.push_back(e);
        else lone.push_back(e);
    }
    auto q = [](std::vector<double> &v, double f) { std::sort(v.begin(), v.end()); return v.empty() ? 0.0 : v[(size_t)(f * (v.size() - 1))]; };
    printf("  %-28s starts p50 %.2f max %.2f; ends min %.2f p10 %.2f p50 %.2f p90 %.2f max %.2f us\n", what, q(st, 0.5), q(st, 1), q(en, 0), q(en, 0.1),
           q(en, 0.5), q(en, 0.9), q(en, 1));
    printf("  %-28s   ends of blockIdx.x <  CUs with a partner (%3zu): p10 %.2f p50 %.2f p90 %.2f max %.2f\n", "", lo.size(), q(lo, 0.1), q(lo, 0.5), q(lo, 0.9), q(lo, 1));
    printf("  %-28s   ends of blockIdx.x >= CUs                (%3zu): p10 %.2f p50 %.2f p90 %.2f max %.2f\n", "", hi.size(), q(hi, 0.1), q(hi, 0.5), q(hi, 0.9), q(hi, 1));
    if (!lone.empty())
        printf("  %-28s   ends of blockIdx.x <  CUs without one    (%3zu): p10 %.2f p50 %.2f p90 %.2f max %.2f\n", "", lone.size(), q(lone, 0.1), q(lone, 0.5), q(lone, 0.9), q(lone, 1));
}

// a launch's length by its stamps: from the first workgroup's start to the last one's end, us
static inline double stamp_span(const std::vector<long long> &ht, int grid) {
    long long t0 = ht[0], t1 = ht[1];
    for (int i = 0; i < grid; ++i) t0 = std::min(t0, ht[2 * i]), t1 = std::max(t1, ht[2 * i + 1]);
    return (t1 - t0) * 0.01;
}
