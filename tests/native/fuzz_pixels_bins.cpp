// Sanitizer harness for the mutual-information rule of the library (csrc/pixels_bins.hpp: the bin of a pixel among a list
// of edges, the score of a joint histogram), built by tests/test_pixels_bins_sanitizers_cpu.py with
// g++ -fsanitize=address,undefined.  Hostile inputs: edge lists of 1 and of 31 entries, edges an ulp apart, huge edges,
// pixels that are NaN, +-inf, exactly on an edge or an ulp beside it, histograms with empty rows and columns, with one
// filled row or column, empty altogether, with cells of 2^31 - 1.  Properties: no sanitizer report (every array is
// allocated to the element), a bin is the number of edges <= the pixel (counted one by one) and lies inside the
// histogram, a NaN pixel gets the NaN code and nothing else does, refused edge lists are the bad ones, and the score --
// computed through the strided entry points the kernel uses -- equals a straightforward second evaluation: NaN for an
// empty histogram, exactly 0.0 for one row or one column, >= 0 and <= log(min(na, nb)) up to rounding, the same bits
// twice and the same bits at any stride.
// usage: fuzz_pixels_bins <iterations> <seed>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>

#include "../../euispice_coreg_amd/csrc/pixels_bins.hpp"

using namespace coreg;

int main(int argc, char** argv) {
    const long iters = argc > 1 ? std::atol(argv[1]) : 2000;
    std::mt19937_64 rng(argc > 2 ? std::atoll(argv[2]) : 1);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    int failures = 0;
    long pixels = 0, scores = 0;
    for (long it = 0; it < iters && failures < 10; ++it) {
        const int kind = (int)(rng() % 8);
        // ---- edges
        const int n = kind == 0 ? 1 : (kind == 1 ? kPixMaxEdges : (int)(rng() % kPixMaxEdges) + 1);
        double* e = (double*)std::malloc(sizeof(double) * n);  // (allocated to the element: ASan guards both ends)
        double c = kind == 2 ? -1e300 : (kind == 3 ? 1e-310 * U(rng) : 100.0 * (2 * U(rng) - 1));
        for (int k = 0; k < n; ++k) {
            e[k] = c;
            c = (kind == 4 || rng() % 3 == 0) ? std::nextafter(c, inf) : c + (kind == 2 ? 1e299 * U(rng) + 1e280 : U(rng) + 1e-9);
        }
        if (!bins_edges_ok(e, n)) {
            std::printf("FAIL it %ld: a good edge list of %d entries is refused\n", it, n);
            ++failures;
        }
        // a spoiled copy is refused: a repeated entry, a falling one, a NaN, an infinity, too many, none
        {
            double* bad = (double*)std::malloc(sizeof(double) * (kPixMaxEdges + 1));
            for (int k = 0; k < kPixMaxEdges + 1; ++k) bad[k] = (double)k;
            bool ok = !bins_edges_ok(bad, kPixMaxEdges + 1) && !bins_edges_ok(bad, 0) && !bins_edges_ok(nullptr, 3) &&
                      bins_edges_ok(bad, kPixMaxEdges);
            const int at = (int)(rng() % kPixMaxEdges);
            const double spoil[4] = {at > 0 ? bad[at - 1] : nan, at > 0 ? bad[at - 1] - 1.0 : -inf, nan, rng() % 2 ? inf : -inf};
            for (int s = 0; s < 4; ++s) {
                const double keep = bad[at];
                bad[at] = spoil[s];
                ok = ok && !bins_edges_ok(bad, kPixMaxEdges);
                bad[at] = keep;
            }
            if (!ok) {
                std::printf("FAIL it %ld: a bad edge list passes (entry %d)\n", it, at);
                ++failures;
            }
            std::free(bad);
        }
        // ---- pixels
        for (int s = 0; s < 64; ++s) {
            double v;
            switch (rng() % 8) {
                case 0: v = nan; break;
                case 1: v = rng() % 2 ? inf : -inf; break;
                case 2: v = e[rng() % n]; break;
                case 3: v = std::nextafter(e[rng() % n], rng() % 2 ? inf : -inf); break;
                case 4: v = rng() % 2 ? 1.7e308 : -1.7e308; break;
                default: v = e[0] + (e[n - 1] - e[0]) * (1.2 * U(rng) - 0.1);
            }
            const int code = bins_code(e, n, v);
            int count = 0;
            for (int k = 0; k < n; ++k) count += e[k] <= v ? 1 : 0;
            const bool isnan = v != v;
            if (isnan ? code != kPixBinNaN : (code != count || code < 0 || code > n || code != bins_index(e, n, v))) {
                std::printf("FAIL it %ld: pixel %.17g among %d edges: code %d, %d edges <= it\n", it, v, n, code, count);
                ++failures;
                break;
            }
            ++pixels;
        }
        // ---- a histogram [na][nb] and its score
        const int na = n + 1, nb = kind == 5 ? 2 : (int)(rng() % (kPixMaxEdges + 1)) + 1;
        const int stride = (int)(rng() % 3) * 8 + 1;  // 1, 9, 17 (the kernel: 16 slots side by side)
        uint32_t* h = (uint32_t*)std::calloc((size_t)na * nb, sizeof(uint32_t));
        uint32_t* hs = (uint32_t*)std::calloc((size_t)na * nb * stride, sizeof(uint32_t));
        const int shape = (int)(rng() % 6);  // 0 empty, 1 one row, 2 one column, 3 sparse with empty rows, 4 dense, 5 one huge cell
        const int one_i = (int)(rng() % na), one_j = (int)(rng() % nb);
        for (int i = 0; i < na; ++i)
            for (int j = 0; j < nb; ++j) {
                uint32_t v = 0;
                if (shape == 1) v = i == one_i ? (uint32_t)(rng() % 1000) : 0;
                if (shape == 2) v = j == one_j ? (uint32_t)(rng() % 1000) : 0;
                if (shape == 3) v = (i % 3 == 1 || rng() % 4) ? 0 : (uint32_t)(rng() % 50000);
                if (shape == 4) v = (uint32_t)(rng() % 100000) + 1;
                if (shape == 5) v = (i == one_i && j == one_j) ? 2147483647u : (uint32_t)(rng() % 2);
                h[i * nb + j] = v;
                hs[(size_t)(i * nb + j) * stride] = v;
            }
        uint32_t* r = (uint32_t*)std::malloc(sizeof(uint32_t) * na);
        uint32_t* cs = (uint32_t*)std::malloc(sizeof(uint32_t) * nb * stride);
        uint32_t* cc = (uint32_t*)std::malloc(sizeof(uint32_t) * nb);
        double* rows = (double*)std::malloc(sizeof(double) * na);
        double* rows_s = (double*)std::malloc(sizeof(double) * na * stride);
        uint32_t total = 0;
        const double got = bins_mi(h, na, nb, r, cc, rows, &total);
        // the kernel's way: margins of its own, a row per call at a stride, the rows summed at a stride
        unsigned long long n_all = 0;
        for (int j = 0; j < nb; ++j) {
            uint32_t v = 0;
            for (int i = 0; i < na; ++i) v += h[i * nb + j];
            cs[(size_t)j * stride] = v;
        }
        for (int i = 0; i < na; ++i) {
            uint32_t v = 0;
            for (int j = 0; j < nb; ++j) v += h[i * nb + j];
            n_all += v;
            if (v != r[i]) {
                std::printf("FAIL it %ld: row sum %d of a %d x %d histogram (shape %d): %u, counted %u\n", it, i, na, nb, shape,
                            r[i], v);
                ++failures;
            }
        }
        for (int i = 0; i < na; ++i)
            rows_s[(size_t)i * stride] = n_all ? bins_mi_row(hs, stride, i, nb, r[i], cs, stride, (uint32_t)n_all) : 0.0;
        const double strided = bins_mi_sum(rows_s, stride, na, (uint32_t)n_all);
        // the straightforward second evaluation: the formula, cell by cell, in long double
        long double want = 0.0L;
        for (int i = 0; i < na; ++i)
            for (int j = 0; j < nb; ++j)
                if (h[i * nb + j]) {
                    const long double nij = h[i * nb + j];
                    want += nij / (long double)n_all * std::log(nij * (long double)n_all / ((long double)r[i] * (long double)cc[j]));
                }
        bool bad = total != (uint32_t)n_all || std::memcmp(&got, &strided, sizeof got) != 0;
        if (n_all == 0)
            bad = bad || got == got;
        else {
            const double lim = std::log((double)(na < nb ? na : nb));
            bad = bad || !(std::fabs(got - (double)want) <= 1e-12) || !(got >= -1e-12 && got <= lim + 1e-12);
            if (shape == 1 || shape == 2) bad = bad || got != 0.0;
        }
        if (bad) {
            std::printf("FAIL it %ld: histogram %d x %d shape %d: score %.17g strided %.17g second evaluation %.17Lg n %llu\n", it,
                        na, nb, shape, got, strided, want, n_all);
            ++failures;
        }
        ++scores;
        std::free(rows_s);
        std::free(rows);
        std::free(cc);
        std::free(cs);
        std::free(r);
        std::free(hs);
        std::free(h);
        std::free(e);
    }
    if (failures) return 1;
    std::printf("ok: %ld iterations, %ld pixels binned, %ld histograms scored\n", iters, pixels, scores);
    return 0;
}
