// The mutual-information rule of the pixel-lag sweep (pxlshift method "mutual_information"), in
// plain C++: the bin of a pixel among a list of edges, and the score of a finished joint histogram.  Host- and
// device-callable: k_pixels_mi (csrc/kernels_pixels_mi.hpp) runs this text per thread, coreg_pixels_set_bins checks its edge
// lists with it, tests/native/fuzz_pixels_bins.cpp runs it under sanitizers on the host.
//
//   bin(v)  = the number of edges e with e <= v            (np.searchsorted(edges, v, side="right"); comparisons only)
//   MI      = sum over n_ij > 0 of (n_ij / n) log((n_ij n) / (r_i c_j))   float64, natural logarithm, nats
//
// with n_ij the integer count of kept pairs in cell (i, j), r_i and c_j its row and column sums and n their total.  The
// terms of a row are added in the order of j from 0, the rows in the order of i from 0: a score is a function of the
// histogram alone.  No function here reads outside its arrays: a bin lies in [0, n_edges], a cell in [0, na) x [0, nb).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define COREG_PB_HD __host__ __device__ __forceinline__
#else
#define COREG_PB_HD inline
#endif

namespace coreg {

constexpr int kPixMaxEdges = 31;   // edges per list at most: 32 bins
constexpr int kPixBinNaN = 255;    // the code of a pixel that is not a number (never a bin: a bin is <= 31)

// an edge list the library takes: 1 to 31 entries, finite, strictly increasing
COREG_PB_HD bool bins_edges_ok(const double* e, int n) {
    if (!e || n < 1 || n > kPixMaxEdges) return false;
    for (int k = 0; k < n; ++k) {
        if (!(fabs(e[k]) < HUGE_VAL)) return false;  // (NaN or infinite)
        if (k > 0 && !(e[k] > e[k - 1])) return false;
    }
    return true;
}

// the number of edges e[k] <= v, by bisection over the strictly increasing list; v is not NaN.  -inf gives 0, +inf gives n
COREG_PB_HD int bins_index(const double* e, int n, double v) {
    int lo = 0, hi = n;  // e[k] <= v for k < lo, e[k] > v for k >= hi
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (e[mid] <= v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// the byte a staged pixel becomes: its bin, or kPixBinNaN
COREG_PB_HD int bins_code(const double* e, int n, double v) { return v == v ? bins_index(e, n, v) : kPixBinNaN; }

// The sum of the terms of row i of a histogram of nb columns, in the order of j.  Cell (i, j) is h[(i * nb + j) * stride],
// c[j * cstride] the column sums, r_i the sum of the row, n the total (> 0).  An empty cell adds nothing.
COREG_PB_HD double bins_mi_row(const uint32_t* h, int stride, int i, int nb, uint32_t r_i, const uint32_t* c, int cstride,
                               uint32_t n) {
#pragma clang fp contract(off)
    double s = 0.0;
    const double dn = (double)n, dr = (double)r_i;
    for (int j = 0; j < nb; ++j) {
        const uint32_t nij = h[(size_t)(i * nb + j) * stride];
        if (nij == 0) continue;
        const double d = (double)nij;
        s = s + (d / dn) * log((d * dn) / (dr * (double)c[(size_t)j * cstride]));
    }
    return s;
}

// the rows added in the order of i; n == 0: NaN
COREG_PB_HD double bins_mi_sum(const double* rows, int stride, int na, uint32_t n) {
#pragma clang fp contract(off)
    if (n == 0) return __builtin_nan("");
    double s = 0.0;
    for (int i = 0; i < na; ++i) s = s + rows[(size_t)i * stride];
    return s;
}

// The score of a whole histogram [na][nb] (stride 1), margins and all: what the kernel computes spread over its threads,
// in one place.  r[na], c[nb], rows[na]: work space.  *n_out: the number of pairs.
COREG_PB_HD double bins_mi(const uint32_t* h, int na, int nb, uint32_t* r, uint32_t* c, double* rows, uint32_t* n_out) {
    uint32_t n = 0;
    for (int j = 0; j < nb; ++j) c[j] = 0;
    for (int i = 0; i < na; ++i) {
        uint32_t s = 0;
        for (int j = 0; j < nb; ++j) {
            s += h[i * nb + j];
            c[j] += h[i * nb + j];
        }
        r[i] = s;
        n += s;
    }
    *n_out = n;
    for (int i = 0; i < na; ++i) rows[i] = n ? bins_mi_row(h, 1, i, nb, r[i], c, 1, n) : 0.0;
    return bins_mi_sum(rows, 1, na, n);
}

}  // namespace coreg
