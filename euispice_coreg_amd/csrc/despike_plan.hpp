// The plan of one median/MAD despiking (coreg_despike_small, coreg_set_reference_despike, coreg_pixels_despike_*, DESIGN
// section 8): the parameter checks with their code and message, the launch geometry -- which work item and thread owns which
// pixel, and where its window stands in the item's LDS -- and the decision itself.  Plain C++ with no HIP dependency:
// included by kernels_despike.hpp (its kernels take their pixels and their decision from the functions below) and used by the
// host parts of libcoreg_hip.so's one translation unit; tests/native/despike_rules.cpp walks it on the host under
// sanitizers, the decision function included: the very arithmetic the GPU runs.
//
// The rule of a pass, for every finite pixel v[j,i] (include/coreg_hip.h states it in full): N = the finite pixels of the
// (2R+1)^2 window clipped to the image, centre left out, as float64, k = |N|; kept when k < min_neighbours; med = median of
// N (the mean of the two middle values for even k, as (a + b) * 0.5), mad = the same selection over |n - med|;
// scale = max(1.4826 * mad, floor), d = v - med; flagged when scale > 0 and d > nsigma * scale (sign = both: |d| > ...).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/coreg_hip.h"

#if defined(__HIPCC__)
#define COREG_DS_HD __host__ __device__ __forceinline__
#else
#define COREG_DS_HD inline
#endif
#if defined(__clang__)
#define COREG_DS_UNROLL _Pragma("unroll")
#else
#define COREG_DS_UNROLL
#endif

namespace coreg {

constexpr int kDespikeMaxR = 3;                                                    // windows up to 7 x 7
constexpr int kDespikeMaxNb = (2 * kDespikeMaxR + 1) * (2 * kDespikeMaxR + 1) - 1;  // 48 neighbours at most
constexpr int kDespikeMaxIter = 8;                                                 // passes of a call at most
constexpr int kDespikeThreads = 256;  // threads of a work item: one pixel each
constexpr int kDespikeTileW = 32;     // a work item is a tile of kDespikeTileW columns (the 32 lanes an LDS read serves
constexpr int kDespikeTileH = 8;      // together read 32 neighbouring float64 of one staged row: one per bank pair)
constexpr long long kDespikeMaxGrid = 65536;  // workgroups of a launch at most: each loops over its work items
static_assert(kDespikeTileW * kDespikeTileH == kDespikeThreads, "one pixel per thread");

constexpr int despike_neighbours(int R) { return (2 * R + 1) * (2 * R + 1) - 1; }

// nullptr: the parameters are good; else what is wrong with them (COREG_EINVAL)
inline const char* despike_params_refusal(const coreg_despike_params* p) {
    if (!p) return "despike: null parameters";
    if (p->radius < 1 || p->radius > kDespikeMaxR) return "despike: radius must be 1, 2 or 3";
    if (p->n_iter < 1 || p->n_iter > kDespikeMaxIter) return "despike: n_iter must be from 1 to 8";
    if (!std::isfinite(p->nsigma) || !(p->nsigma > 0.0)) return "despike: nsigma must be finite and positive";
    if (!std::isfinite(p->floor) || p->floor < 0.0) return "despike: floor must be finite and not negative";
    if (p->min_neighbours < 1 || p->min_neighbours > despike_neighbours(p->radius))
        return "despike: min_neighbours must be from 1 to (2 radius + 1)^2 - 1";
    if (p->sign != COREG_DESPIKE_POSITIVE && p->sign != COREG_DESPIKE_BOTH) return "despike: sign must be positive (0) or both (1)";
    if (p->replace != COREG_DESPIKE_NAN && p->replace != COREG_DESPIKE_MEDIAN) return "despike: replace must be nan (0) or median (1)";
    return nullptr;
}

// ---- geometry: shared by the kernel and the host -------------------------------------------------------------------------
struct DespikeGeom {
    int W, H;         // the image
    int n_tx, n_ty;   // tiles per row of tiles, rows of tiles
    long long items;  // n_ty x n_tx
};

// the first row / column of the item's tile
COREG_DS_HD void despike_origin(const DespikeGeom& g, long long item, int* y0, int* x0) {
    *y0 = (int)(item / g.n_tx) * kDespikeTileH;
    *x0 = (int)(item % g.n_tx) * kDespikeTileW;
}
// the pixel thread t of work item `item` owns; false: none (outside the image; the coordinate past the end is H or W then)
// (sums of a coordinate and an offset are 64-bit throughout: a row or column may have close to 2^31 pixels)
COREG_DS_HD bool despike_pixel(const DespikeGeom& g, long long item, int t, int* row, int* col) {
    int y0, x0;
    despike_origin(g, item, &y0, &x0);
    const long long r = (long long)y0 + t / kDespikeTileW, c = (long long)x0 + t % kDespikeTileW;
    *row = (int)(r < g.H ? r : g.H);
    *col = (int)(c < g.W ? c : g.W);
    return r < g.H && c < g.W;
}
// the staged window of an item: the tile and an R-wide halo, float64, rows of despike_lds_pitch(R) entries; entry e stands
// for the pixel (y0 - R + e / pitch, x0 - R + e % pitch), NaN where that is not finite or outside the image
COREG_DS_HD constexpr int despike_lds_pitch(int R) { return kDespikeTileW + 2 * R; }
COREG_DS_HD constexpr int despike_lds_rows(int R) { return kDespikeTileH + 2 * R; }
COREG_DS_HD constexpr int despike_lds_entries(int R) { return despike_lds_pitch(R) * despike_lds_rows(R); }
COREG_DS_HD constexpr size_t despike_lds_bytes(int R) { return (size_t)despike_lds_entries(R) * sizeof(double); }
// where thread t reads the neighbour (dy, dx) of its pixel, |dy|, |dx| <= R
COREG_DS_HD constexpr int despike_lds_index(int R, int t, int dy, int dx) {
    return (t / kDespikeTileW + R + dy) * despike_lds_pitch(R) + (t % kDespikeTileW + R + dx);
}

// A refusal (code != COREG_OK, msg) or what the launch of a pass needs
struct DespikePlan {
    int code = COREG_OK;
    const char* msg = nullptr;
    DespikeGeom g = {};
    unsigned grid = 0;  // workgroups: min(items, kDespikeMaxGrid)
    size_t lds = 0;     // LDS of an item (static in k_despike_image<T, R>)
};

inline DespikePlan despike_plan(long long H, long long W, const coreg_despike_params* prm) {
    DespikePlan p;
    const char* why = despike_params_refusal(prm);
    if (!why && (H < 1 || W < 1 || H > 2147483647ll / W)) why = "despike: empty image, or more than 2^31 - 1 pixels";
    if (why) {
        p.code = COREG_EINVAL;
        p.msg = why;
        return p;
    }
    DespikeGeom& g = p.g;
    g.W = (int)W;
    g.H = (int)H;
    g.n_tx = (int)((W + kDespikeTileW - 1) / kDespikeTileW);  // (64-bit: W + 31 may pass 2^31)
    g.n_ty = (int)((H + kDespikeTileH - 1) / kDespikeTileH);
    g.items = (long long)g.n_ty * g.n_tx;
    p.grid = (unsigned)std::min(g.items, kDespikeMaxGrid);
    p.lds = despike_lds_bytes(prm->radius);
    return p;
}

// ---- the decision: shared by the kernel and the host ---------------------------------------------------------------------
struct DespikeDecision {
    bool flagged;
    double med;  // the median of the neighbours (0 when there were fewer than min_neighbours)
};

// Batcher's odd-even merge sort of P = 2^m entries, ascending, as a fixed network of compare-exchanges (19 for P = 8, 191
// for 32, 543 for 64): comparisons and selections only, no data-dependent branch, the same instructions for every lane.
// Constant trip counts and indices: the loops unroll and s[] stays in registers.  (Chosen by measurement against rank
// counting -- for every entry, how many lie below it and how many at or below it -- which gave the same bits and took
// 2.8 to 3 times as long at 24 and 48 entries: DESIGN section 8, Q26.)
template <int P>
COREG_DS_HD void despike_sort(double (&s)[P]) {
    COREG_DS_UNROLL
    for (int p = 1; p < P; p *= 2) {
        COREG_DS_UNROLL
        for (int k = p; k >= 1; k /= 2) {
            COREG_DS_UNROLL
            for (int j = k % p; j <= P - 1 - k; j += 2 * k) {
                COREG_DS_UNROLL
                for (int i = 0; i <= (k - 1 < P - j - k - 1 ? k - 1 : P - j - k - 1); ++i) {
                    if ((i + j) / (p * 2) == (i + j + k) / (p * 2)) {
                        const double x = s[i + j], y = s[i + j + k];
                        const bool swap = y < x;
                        s[i + j] = swap ? y : x;
                        s[i + j + k] = swap ? x : y;
                    }
                }
            }
        }
    }
}

// The values at the positions pos_lo and pos_hi (0-based, below the number of entries that are not NaN) of the entries of
// a[NN] that are not NaN, in ascending order; NaN entries stand for "no neighbour".  They and the padding to a power of two
// sort as +Inf, behind every value (an |n - med| that overflowed is +Inf too, and equal to them: the value is the same).
template <int NN>
COREG_DS_HD void despike_select2(const double (&a)[NN], int pos_lo, int pos_hi, double* lo, double* hi) {
    constexpr int P = NN <= 8 ? 8 : NN <= 32 ? 32 : 64;
    static_assert(NN <= P, "at most 64 entries");
    double s[P];
    COREG_DS_UNROLL
    for (int i = 0; i < P; ++i) {
        const double v = a[i < NN ? i : 0];
        s[i] = (i < NN && v == v) ? v : HUGE_VAL;
    }
    despike_sort<P>(s);
    double vlo = 0.0, vhi = 0.0;
    COREG_DS_UNROLL
    for (int i = 0; i < NN; ++i) {  // (a run-time index into s[] would send it to scratch)
        if (i == pos_lo) vlo = s[i];
        if (i == pos_hi) vhi = s[i];
    }
    *lo = vlo;
    *hi = vhi;
}

// median of the k >= 1 finite entries of a[NN]: s[k/2] for odd k, (s[k/2 - 1] + s[k/2]) * 0.5 for even k
template <int NN>
COREG_DS_HD double despike_median(const double (&a)[NN], int k) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double lo, hi;
    despike_select2<NN>(a, (k & 1) ? k / 2 : k / 2 - 1, k / 2, &lo, &hi);
    return (k & 1) ? hi : (lo + hi) * 0.5;
}

// The centre value c (finite) and its NN = (2R+1)^2 - 1 neighbour slots n[] as float64, NaN in every slot that holds no
// finite pixel of the image.  The four float operations are each rounded on their own (no contraction).
template <int NN>
COREG_DS_HD DespikeDecision despike_decide(double c, const double (&n)[NN], const coreg_despike_params& p) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    int k = 0;
    COREG_DS_UNROLL
    for (int i = 0; i < NN; ++i) k += n[i] == n[i] ? 1 : 0;
    DespikeDecision out = {false, 0.0};
    if (k < p.min_neighbours) return out;  // (min_neighbours >= 1: k >= 1 below)
    const double med = despike_median<NN>(n, k);
    double dev[NN];
    COREG_DS_UNROLL
    for (int i = 0; i < NN; ++i) dev[i] = std::fabs(n[i] - med);  // (NaN stays NaN)
    const double mad = despike_median<NN>(dev, k);
    const double s = 1.4826 * mad;
    const double scale = s > p.floor ? s : p.floor;
    const double d = c - med;
    const double lim = p.nsigma * scale;
    out.med = med;
    out.flagged = scale > 0.0 && (p.sign == COREG_DESPIKE_BOTH ? std::fabs(d) > lim : d > lim);
    return out;
}

}  // namespace coreg
