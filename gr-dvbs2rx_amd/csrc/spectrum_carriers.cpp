// spectrum_carriers.cpp -- the carrier finder over one row of a power spectrum (spectrum_hip.h). Host only, double arithmetic,
// deterministic; tests/spectrum_model.py restates it operation by operation.
//
// The row is taken in frequency order, y[i] the bin of frequency (i - nfft / 2) / nfft cycles per sample, and is circular throughout.
//   1. sm[i] = (sum over d = -(smooth - 1) / 2 .. (smooth - 1) / 2, ascending, of y[i + d]) / smooth.
//   2. floor = sorted(sm)[floor(floor_quantile (nfft - 1))]; thr = floor 10^(threshold_db / 10); a bin is up when sm[i] > thr.
//   3. The walk starts behind the longest run of bins that are not up (the first of them in index order). Runs of up bins are regions;
//      two regions with fewer than min_gap bins between them become one; regions of fewer than min_width bins are dropped. No bin up,
//      or no run of min_gap bins that are not up: nothing is found.
//   4. Per region [a, b) with e[u] = sm[u] - floor: centre, the centroid sum e[u] u / sum e[u] over the region and its skirts (outwards
//      on either side while e stays positive, at most half way to the neighbouring region: a region cut at the threshold is lopsided by
//      up to a bin when the carrier sits between two bin centres, and so would its centroid be); level, the median of e over
//      [a + w / 4, b - w / 4), w = b - a; bandwidth, the distance between the two places where e, followed outwards from that middle
//      half, first falls below level / 2, linearly interpolated between the two bins (the region's width where it never does).
#include "spectrum_hip.h"
#include <algorithm>
#include <cmath>

namespace dvbs2 {

std::string spectrum_carriers_check(const float* psd, int nfft, const SpectrumCarrierParams& p)
{
    if (nfft < 16 || nfft > (1 << 20) || (nfft & (nfft - 1))) return "nfft must be a power of two in 16..2^20";
    if (!psd) return "psd is null";
    if (p.smooth < 1 || !(p.smooth & 1) || p.smooth > nfft / 2) return "smooth must be odd and in 1..nfft/2";
    if (!(p.floor_quantile >= 0.0 && p.floor_quantile <= 1.0)) return "floor_quantile must be in 0..1";
    if (!(p.threshold_db > 0.0 && p.threshold_db <= 200.0)) return "threshold_db must be above 0 and at most 200";
    if (p.min_gap < 1 || p.min_gap > nfft) return "min_gap must be in 1..nfft";
    if (p.min_width < 1 || p.min_width > nfft) return "min_width must be in 1..nfft";
    for (int i = 0; i < nfft; i++)
        if (!std::isfinite(psd[i]) || psd[i] < 0.0f) return "psd[" + std::to_string(i) + "] is negative or not finite";
    return "";
}

std::vector<SpectrumCarrier> spectrum_carriers(const float* psd, int nfft, bool shifted, const SpectrumCarrierParams& p)
{
    std::vector<SpectrumCarrier> found;
    const int N = nfft, mask = N - 1, rot = shifted ? 0 : N / 2; // y[i] = psd[(i + rot) mod N]
    std::vector<double> sm((size_t)N);
    const int h = (p.smooth - 1) / 2;
    for (int i = 0; i < N; i++) {
        double s = 0.0;
        for (int d = -h; d <= h; d++) s += (double)psd[(i + d + rot + N) & mask];
        sm[(size_t)i] = s / p.smooth;
    }
    std::vector<double> sorted(sm);
    std::sort(sorted.begin(), sorted.end());
    const double floor_level = sorted[(size_t)std::floor(p.floor_quantile * (N - 1))];
    const double thr = floor_level * std::pow(10.0, p.threshold_db / 10.0);
    auto up = [&](int u) { return sm[(size_t)(u & mask)] > thr; };

    // the longest run of bins that are not up, the first in index order among equals; circular: a run may pass the end
    int best_start = -1, best_len = 0;
    for (int i = 0; i < N; i++) {
        if (up(i) || !up(i - 1 + N)) continue; // i starts a run
        int len = 1;
        while (len < N && !up(i + len)) len++;
        if (len > best_len) { best_len = len; best_start = i; }
    }
    if (best_start < 0) return found; // every bin up, or none (then the row has no run's start either)
    if (best_len < p.min_gap) return found;

    // regions in unwrapped coordinates u in [u0, u0 + N), u0 behind the longest gap
    const int u0 = best_start + best_len;
    std::vector<std::pair<int, int>> regions; // [a, b)
    for (int u = u0; u < best_start + N;) {
        if (!up(u)) { u++; continue; }
        int b = u;
        while (b < best_start + N && up(b)) b++;
        if (!regions.empty() && u - regions.back().second < p.min_gap) regions.back().second = b;
        else regions.emplace_back(u, b);
        u = b;
    }
    const int nr = (int)regions.size();
    for (int r = 0; r < nr; r++) {
        const int a = regions[(size_t)r].first, b = regions[(size_t)r].second, w = b - a;
        if (w < p.min_width) continue;
        auto e = [&](int u) { return sm[(size_t)(u & mask)] - floor_level; };
        // the centroid takes the skirts along: outwards while e stays positive, at most half way to the neighbouring region
        const int before = r > 0 ? regions[(size_t)r - 1].second : regions[(size_t)nr - 1].second - N;
        const int behind = r + 1 < nr ? regions[(size_t)r + 1].first : regions[0].first + N;
        const int lo_limit = a - (a - before) / 2, hi_limit = b + (behind - b) / 2;
        int ca = a, cb = b;
        while (ca > lo_limit && e(ca - 1) > 0.0) ca--;
        while (cb < hi_limit && e(cb) > 0.0) cb++;
        double se = 0.0, su = 0.0;
        for (int u = ca; u < cb; u++) { se += e(u); su += e(u) * (double)u; }
        const int m0 = a + w / 4, m1 = b - w / 4; // the middle half [m0, m1), not empty
        std::vector<double> mid;
        for (int u = m0; u < m1; u++) mid.push_back(e(u));
        std::sort(mid.begin(), mid.end());
        const size_t k = mid.size();
        const double level = k & 1 ? mid[k / 2] : 0.5 * (mid[k / 2 - 1] + mid[k / 2]);
        const double half = 0.5 * level;
        double xl = (double)a, xr = (double)b;
        bool have = level > 0.0;
        if (have) {
            int u = m0;
            while (u > m0 - N && e(u) >= half) u--;
            int v = m1 - 1;
            while (v < m1 - 1 + N && e(v) >= half) v++;
            have = e(u) < half && e(v) < half;
            if (have) {
                xl = (double)u + (half - e(u)) / (e(u + 1) - e(u));
                xr = (double)v - (half - e(v)) / (e(v - 1) - e(v));
            }
        }
        SpectrumCarrier c;
        double f = (su / se) / (double)N - 0.5;
        f -= std::floor(f + 0.5);
        c.centre = f;
        c.bandwidth = (xr - xl) / (double)N;
        c.level = level;
        c.floor = floor_level;
        c.lo_bin = (a + rot) & mask;
        c.hi_bin = (b - 1 + rot) & mask;
        found.push_back(c);
    }
    std::stable_sort(found.begin(), found.end(), [](const SpectrumCarrier& x, const SpectrumCarrier& y) { return x.centre < y.centre; });
    return found;
}

} // namespace dvbs2
