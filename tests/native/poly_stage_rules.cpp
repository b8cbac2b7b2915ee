// The last axis of a spline sample as a polynomial in its fraction (csrc/spline_last.hpp: spline_last_o1 / _o2 / _o3),
// compiled for the host -- the very functions the kernels run -- and held to
//   * a long double evaluation of scipy's weights (ni_splines.c, get_spline_interpolation_weights) applied to the same
//     row sums, at the scale the functions work at: order 2 doubled weights, order 3 six-fold row sums and 1/36;
//   * the weight form the kernels used before (restated here: weights in double, a column of fma, the final scale),
//     against the same reference on the same inputs: the polynomial forms its coefficients from differences of the row
//     sums, which cancel, so it is allowed TWICE the weight form's maximum error, no more.  Both maxima are printed.
//   * non-finite row sums: every assignment of {finite, NaN, +inf, -inf} to the rows with at least one non-finite gives
//     a non-finite result at EVERY fraction (the sample mask of k_sweep relies on it).
// Error of one evaluation: |got - reference| / max_r |R_r| -- the scale both forms are backward stable to; the result
// itself may cancel to nothing under rows of mixed sign.
// Fractions: 0, 2^-53, 1/2, 1 - 2^-53 and a seeded random set; row sums: seeded, mixed sign and scale.
// Host compiler only, -ffp-contract=off (the restated weight form must not be fused); prints "ok: ..." and returns 0.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../../euispice_coreg_amd/csrc/spline_last.hpp"

namespace {
int n_bad = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            if (++n_bad <= 20) {               \
                std::printf("FAIL: " __VA_ARGS__); \
                std::printf("\n");             \
            }                                  \
        }                                      \
    } while (0)

// ---- scipy's weights in long double ------------------------------------------------------------------------------------
// f: the argument counted from the first tap, [0, 1).  Order 2: scipy's argument is t = f - 1/2 about the middle tap.
void scipy_weights(int order, long double f, long double* w) {
    if (order == 1) {
        w[0] = 1.0L - f;
        w[1] = f;
    } else if (order == 2) {
        const long double t = f - 0.5L;
        w[1] = 0.75L - t * t;
        const long double y = 0.5L - t;
        w[0] = 0.5L * y * y;
        w[2] = 1.0L - w[0] - w[1];
    } else {
        const long double z = 1.0L - f;
        w[1] = (f * f * (f - 2.0L) * 3.0L + 4.0L) / 6.0L;
        w[2] = (z * z * (z - 2.0L) * 3.0L + 4.0L) / 6.0L;
        w[0] = z * z * z / 6.0L;
        w[3] = 1.0L - w[0] - w[1] - w[2];
    }
}
// the sample at the scale of spline_last_oN: order 2 doubled, order 3 six-fold rows -> / 6
long double reference(int order, const double* r, double f) {
    long double w[4], v = 0.0L;
    scipy_weights(order, (long double)f, w);
    for (int k = 0; k <= order; ++k) v += w[k] * (long double)r[k];
    return order == 2 ? 2.0L * v : order == 3 ? v / 6.0L : v;
}

// ---- the weight form of before, restated -------------------------------------------------------------------------------
double weight_form(int order, const double* r, double f) {
    double w[4], v = 0.0;
    if (order == 1) {
        w[0] = 1.0 - f;
        w[1] = f;
    } else if (order == 2) {  // doubled: g^2, 1 + 2 f g, f^2
        const double g = 1.0 - f;
        w[0] = g * g;
        w[2] = f * f;
        w[1] = (2.0 - w[0]) - w[2];
    } else {  // six-fold
        const double z = 1.0 - f;
        const double y2 = f * f, z2 = z * z;
        w[0] = z2 * z;
        w[1] = std::fma(3.0 * y2, f - 2.0, 4.0);
        w[2] = std::fma(3.0 * z2, z - 2.0, 4.0);
        w[3] = ((6.0 - w[0]) - w[1]) - w[2];
    }
    for (int k = 0; k <= order; ++k) v = std::fma(r[k], w[k], v);
    return order == 3 ? v * (1.0 / 36.0) : v;
}

double poly_form(int order, const double* r, double f) {
    if (order == 1) return coreg::spline_last_o1(r[0], r[1], f);
    // the gathers hand over R0 + R1 (order 2) and R0 + R2 (order 3), which they get by starting one row's accumulation
    // from the other's sum (spline_chain_row): one rounding, as here
    if (order == 2) return coreg::spline_last_o2(r[0], r[0] + r[1], r[2], f);
    return coreg::spline_last_o3(r[0], r[1], r[0] + r[2], r[3], f);
}
}  // namespace

int main() {
    std::mt19937_64 rng(20240611);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    std::vector<double> fr = {0.0, std::ldexp(1.0, -53), 0.5, 1.0 - std::ldexp(1.0, -53)};
    for (int k = 0; k < 1500; ++k) fr.push_back(uni(rng));
    for (int k = 0; k < 250; ++k) fr.push_back(std::ldexp(uni(rng), -(int)(rng() % 40)));        // towards 0
    for (int k = 0; k < 250; ++k) fr.push_back(1.0 - std::ldexp(uni(rng), -1 - (int)(rng() % 40)));  // towards 1
    for (double f : fr) CHECK(f >= 0.0 && f < 1.0, "fraction %.17g outside [0, 1)", f);

    // row sums: mixed sign; scales from "all alike" to twelve decades apart; smooth rows (neighbouring pixels) too
    std::vector<std::vector<double>> rows;
    for (int k = 0; k < 300; ++k) {
        std::vector<double> r(4);
        const int kind = k % 3;
        const double base = std::pow(10.0, 6.0 * uni(rng) - 3.0) * (rng() & 1 ? 1.0 : -1.0);
        for (int j = 0; j < 4; ++j) {
            if (kind == 0) r[j] = std::pow(10.0, 12.0 * uni(rng) - 6.0) * (rng() & 1 ? 1.0 : -1.0);
            else if (kind == 1) r[j] = (2.0 * uni(rng) - 1.0) * std::fabs(base);
            else r[j] = base * (1.0 + 1e-3 * (2.0 * uni(rng) - 1.0));
        }
        rows.push_back(r);
    }

    // which sums the gathers form (the functions above are written for exactly these)
    for (int order = 1; order <= 3; ++order)
        for (int r = 0; r <= order; ++r)
            CHECK(coreg::spline_chain_row(order, r) == ((order == 2 && r == 1) || (order == 3 && r == 2) ? 0 : -1),
                  "spline_chain_row(%d, %d)", order, r);
    for (int order = 1; order <= 3; ++order) {
        double worst_w = 0.0, worst_p = 0.0;
        for (const auto& r : rows) {
            double scale = 0.0;
            for (int k = 0; k <= order; ++k) scale = std::fmax(scale, std::fabs(r[k]));
            for (double f : fr) {
                const long double want = reference(order, r.data(), f);
                const double ew = (double)(fabsl((long double)weight_form(order, r.data(), f) - want) / scale);
                const double ep = (double)(fabsl((long double)poly_form(order, r.data(), f) - want) / scale);
                worst_w = std::fmax(worst_w, ew);
                worst_p = std::fmax(worst_p, ep);
            }
        }
        std::printf("order %d: max error / max|R|  weight form %.3e  polynomial %.3e  (ratio %.2f, allowed 2)\n", order,
                    worst_w, worst_p, worst_p / worst_w);
        CHECK(worst_w > 0.0 && worst_w < 1e-14, "order %d: the weight form itself is off (%.3e)", order, worst_w);
        CHECK(worst_p <= 2.0 * worst_w, "order %d: polynomial %.3e > 2 x weight form %.3e", order, worst_p, worst_w);
        // the two-step form of order 3 (the gather computes f / 3 and f / 12 ahead) is the same arithmetic
        if (order == 3)
            for (double f : fr) {
                double f3, f12;
                coreg::spline_last_o3_fractions(f, f3, f12);
                const auto& r = rows[0];
                const double a = coreg::spline_last_o3(r[0], r[1], r[0] + r[2], r[3], f, f3, f12);
                const double b = coreg::spline_last_o3(r[0], r[1], r[0] + r[2], r[3], f);
                CHECK(a == b, "order 3: the two forms differ at f = %.17g", f);
            }

        // non-finite row sums: 0 finite, 1 NaN, 2 +inf, 3 -inf per row, every assignment but the all-finite one
        const double special[4] = {0.0, std::nan(""), INFINITY, -INFINITY};
        const int n = order + 1;
        long long n_cases = 0;
        for (int code = 1; code < (1 << (2 * n)); ++code) {
            for (int variant = 0; variant < 3; ++variant) {
                double r[4];
                for (int k = 0; k < n; ++k) {
                    const int c = (code >> (2 * k)) & 3;
                    r[k] = c ? special[c] : rows[(size_t)(code + 7 * variant) % rows.size()][k];
                }
                for (double f : fr) {
                    const double v = poly_form(order, r, f);
                    ++n_cases;
                    CHECK(!std::isfinite(v), "order %d: rows code %d at f = %.17g give the finite %.17g", order, code, f, v);
                    if (order == 3) {
                        double f3, f12;
                        coreg::spline_last_o3_fractions(f, f3, f12);
                        CHECK(!std::isfinite(coreg::spline_last_o3(r[0], r[1], r[0] + r[2], r[3], f, f3, f12)),
                              "order 3 (fractions ahead): rows code %d at f = %.17g finite", code, f);
                    }
                }
            }
        }
        std::printf("order %d: %lld evaluations with a non-finite row sum, none finite\n", order, n_cases);
    }
    if (n_bad) {
        std::printf("%d failure(s)\n", n_bad);
        return 1;
    }
    std::printf("ok: 3 orders, %zu fractions x %zu row sets\n", fr.size(), rows.size());
    return 0;
}
