// Part of csrc/kernels_common.hpp (included from there): the LAST axis of a separable B-spline sample, evaluated as a
// polynomial in the fraction of its coordinate.  Plain C++ with no HIP dependency, so that the host can compile the
// very functions the kernels run (tests/native/poly_stage_rules.cpp).
//
// A sample is sum_r wy[r] * R_r, R_r = sum_c wx[c] * tap[r][c] the row sums.  The x-weights serve every row and stay
// weights; the y-weights serve that one sum, which is a polynomial of degree `order` in the fraction f of the
// y-coordinate with differences of the row sums as coefficients.  Written that way it needs neither 1 - f nor any
// weight.  One SUM of two rows comes for nothing where a row's accumulation starts from another row's sum instead of
// from its first product (an fma in the place of a multiplication: spline_chain_row), and the polynomials are written
// in terms of it: 2 instructions against 3 (order 1), 6 against 8 (order 2), 12 against 18 (order 3, the final scale
// included).
//
// f is what scipy's ni_splines.c calls the spline argument, counted from the FIRST tap's side: order 1 and 3
// f = c - floor(c), order 2 f = (c + 1/2) - floor(c + 1/2), always in [0, 1).
//
// Non-finite taps.  A NaN or an infinity among the taps makes its row sum NaN or infinite (the x-weights are finite;
// 0 * inf is NaN), a chained sum likewise when either of its rows has one (inf - inf is NaN), and every function below
// returns NaN or an infinity when one of its row arguments is one, at EVERY f, so that the sample mask drops the sample
// exactly where a weight form does:
//   * the result is fma(., ., q) with q a sum of finite multiples of all rows but the last; q is NaN or infinite when
//     one of those rows is, and fma(x, y, NaN or inf) is never finite;
//   * the last row enters through the highest coefficient alone: that coefficient is then NaN or infinite, and the
//     chain multiplies it by f (or f / 3): 0 * inf = NaN at f = 0, an infinity or NaN otherwise, which every later
//     fma keeps non-finite.
// Nothing else is done to a row sum: one that was finite stays finite.
#pragma once
#include <cmath>
#if defined(__HIPCC__)
#define COREG_HD __host__ __device__
#else
#define COREG_HD
#endif
namespace coreg {

// the row whose sum row `r` of an order's gather starts its accumulation from (-1: from nothing): order 2 hands
// spline_last_o2 R0 + R1 in the place of R1, order 3 hands spline_last_o3 R0 + R2 in the place of R2
COREG_HD constexpr int spline_chain_row(int order, int r) {
    return (order == 2 && r == 1) || (order == 3 && r == 2) ? 0 : -1;
}

// order 1: (1 - f) R0 + f R1
COREG_HD inline double spline_last_o1(double r0, double r1, double f) { return std::fma(f, r1 - r0, r0); }

// order 2, weights DOUBLED (they sum to 2): g^2 R0 + (1 + 2 f g) R1 + f^2 R2 with g = 1 - f
//   = (R0 + R1) + f (2 (R1 - R0) + f (R0 - 2 R1 + R2)),     from R0, s01 = R0 + R1 and R2:
//   u = R1 - R0 = s01 - 2 R0,  c = R0 - 2 R1 + R2 = (R2 - R0) - 2 u,  v = (s01 + f u) + f (u + f c)
// The caller's row sums carry the factor 1/2: on the LDS path the window holds pixel / 4 under doubled x-weights
// (gather_o2), on the global-memory path the x-weights are halved (Spline<2>::eval_x).
COREG_HD inline double spline_last_o2(double r0, double s01, double r2, double f) {
    const double u = std::fma(-2.0, r0, s01);
    const double c = std::fma(-2.0, u, r2 - r0);
    const double a = std::fma(f, u, s01);
    const double b = std::fma(f, c, u);
    return std::fma(f, b, a);
}

// order 3 from SIX-FOLD row sums (x-weights of spline_weights6_o3), the 1/36 of both axes folded into the constants:
//   36 v = (R0 + 4 R1 + R2) + 3 f ((R2 - R0) + f ((R0 - 2 R1 + R2) + (f / 3) (R3 - R0 + 3 (R1 - R2)))),
// from R0, R1, s02 = R0 + R2 and R3 (R2 - R0 = s02 - 2 R0; R3 - R0 + 3 (R1 - R2) = R3 + 2 R0 + 3 R1 - 3 s02).
// f3 = f / 3 and f12 = f / 12 depend on the coordinate alone: the gather computes them under the latency of its reads.
COREG_HD inline double spline_last_o3(double r0, double r1, double s02, double r3, double f, double f3, double f12) {
    const double a = std::fma(4.0, r1, s02);
    const double c = std::fma(-2.0, r1, s02);
    const double b = std::fma(-2.0, r0, s02);
    const double d = std::fma(-3.0, s02, std::fma(3.0, r1, std::fma(2.0, r0, r3)));
    const double h = std::fma(f, std::fma(f3, d, c), b);
    return std::fma(f12, h, a * (1.0 / 36.0));
}
COREG_HD inline void spline_last_o3_fractions(double f, double& f3, double& f12) {
    f3 = f * (1.0 / 3.0);
    f12 = f * (1.0 / 12.0);
}
COREG_HD inline double spline_last_o3(double r0, double r1, double s02, double r3, double f) {
    double f3, f12;
    spline_last_o3_fractions(f, f3, f12);
    return spline_last_o3(r0, r1, s02, r3, f, f3, f12);
}

}  // namespace coreg
