// Sanitizer harness for the destretch rule of the library (csrc/pixels_field.hpp: the displacement of a local shift field
// at an output pixel, the taps and weights of the order-1 sample), built by tests/test_pixels_field_sanitizers_cpu.py with
// g++ -fsanitize=address,undefined.  Hostile fields: one node on an axis, ragged centres, pixels far outside the field,
// huge offsets, huge node values, planes of one row or one column.  Properties: no sanitizer report (every array is
// allocated to the element), cell indices in [0, n - 1], fractions in [0, 1], tap indices inside the plane, weights in
// [0, 1], the displacement within the range of the nodes, the same bits twice.
// usage: fuzz_pixels_field <iterations> <seed>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../../euispice_coreg_amd/csrc/pixels_field.hpp"

using namespace coreg;

int main(int argc, char** argv) {
    const long iters = argc > 1 ? std::atol(argv[1]) : 2000;
    std::mt19937_64 rng(argc > 2 ? std::atoll(argv[2]) : 1);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    int failures = 0;
    long samples = 0;
    for (long it = 0; it < iters && failures < 10; ++it) {
        const int kind = (int)(rng() % 8);
        PixField f;
        f.n_ty = kind == 1 ? 1 : (int)(rng() % 6) + 1;
        f.n_tx = kind == 2 ? 1 : (int)(rng() % 7) + 1;
        f.th = (int)(rng() % 9) + 1;
        f.tw = (int)(rng() % 9) + 1;
        f.interp = (int)(rng() % 2);
        double* ys = (double*)std::malloc(sizeof(double) * f.n_ty);  // (allocated to the element: ASan guards both ends)
        double* xs = (double*)std::malloc(sizeof(double) * f.n_tx);
        double* u = (double*)std::malloc(sizeof(double) * f.n_ty * f.n_tx);
        double* v = (double*)std::malloc(sizeof(double) * f.n_ty * f.n_tx);
        // centres of tiles th x tw, the last one ragged (kind 3: any strictly increasing centres, a hair apart at places)
        for (int k = 0; k < f.n_ty; ++k) ys[k] = k * f.th + (f.th - 1) / 2.0;
        for (int k = 0; k < f.n_tx; ++k) xs[k] = k * f.tw + (f.tw - 1) / 2.0;
        if (f.n_ty > 1) ys[f.n_ty - 1] -= 0.5 * (double)(rng() % f.th);
        if (f.n_tx > 1) xs[f.n_tx - 1] -= 0.5 * (double)(rng() % f.tw);
        if (kind == 3) {
            double c = -1e6 * U(rng);
            for (int k = 0; k < f.n_tx; ++k) xs[k] = c = (rng() % 3 ? std::nextafter(c, 1e300) : c + 1e5 * U(rng) + 1e-9);
        }
        const double amp = kind == 4 ? 1e300 : (kind == 5 ? 1e-300 : 6.0);
        double lo[2] = {1e308, 1e308}, hi[2] = {-1e308, -1e308};
        for (int k = 0; k < f.n_ty * f.n_tx; ++k) {
            u[k] = amp * (2 * U(rng) - 1);
            v[k] = rng() % 4 ? amp * (2 * U(rng) - 1) : (double)((int)(rng() % 7) - 3);
            lo[0] = std::fmin(lo[0], u[k]), hi[0] = std::fmax(hi[0], u[k]);
            lo[1] = std::fmin(lo[1], v[k]), hi[1] = std::fmax(hi[1], v[k]);
        }
        f.ys = ys, f.xs = xs, f.u = u, f.v = v;
        f.row_offset = kind == 6 ? 1e300 * (2 * U(rng) - 1) : (double)((int)(rng() % 21) - 10);
        f.col_offset = kind == 6 ? -1.7e308 * U(rng) : (double)((int)(rng() % 21) - 10);
        const int W = kind == 7 ? 1 : (int)(rng() % 40) + 1, H = rng() % 5 ? (int)(rng() % 30) + 1 : 1;
        float* img = (float*)std::malloc(sizeof(float) * W * H);
        for (int k = 0; k < W * H; ++k) img[k] = rng() % 11 ? (float)U(rng) : std::nanf("");
        for (int s = 0; s < 64; ++s) {
            // output pixels of the plane, and pixels far outside it (the rule itself must hold anywhere)
            const double far = s % 8 == 7 ? 1e12 * (2 * U(rng) - 1) : 0.0;
            const double X = (double)(rng() % W) + far, Y = (double)(rng() % H) - far;
            // the cells behind the displacement
            int i0, i1, j0, j1;
            double fx, fy;
            field_cell(xs, f.n_tx, X - f.col_offset, &i0, &i1, &fx);
            field_cell(ys, f.n_ty, Y - f.row_offset, &j0, &j1, &fy);
            const int ti = field_tile(X - f.col_offset, f.tw, f.n_tx), tj = field_tile(Y - f.row_offset, f.th, f.n_ty);
            if (i0 < 0 || i1 >= f.n_tx || i1 < i0 || i1 - i0 > 1 || j0 < 0 || j1 >= f.n_ty || j1 < j0 || j1 - j0 > 1 ||
                !(fx >= 0.0 && fx <= 1.0 && fy >= 0.0 && fy <= 1.0) || ti < 0 || ti >= f.n_tx || tj < 0 || tj >= f.n_ty) {
                std::printf("FAIL it %ld: cell (%d %d %g) (%d %d %g) tile (%d %d) of %d x %d nodes\n", it, i0, i1, fx, j0, j1, fy,
                            tj, ti, f.n_ty, f.n_tx);
                ++failures;
                break;
            }
            double d[2], e[2];
            field_displacement(f, X, Y, &d[0], &d[1]);
            field_displacement(f, X, Y, &e[0], &e[1]);
            bool bad = std::memcmp(d, e, sizeof d) != 0;
            for (int k = 0; k < 2; ++k) {  // a convex combination of the nodes, up to rounding
                const double slack = 1e-12 * std::fmax(std::fabs(lo[k]), std::fabs(hi[k]));
                bad = bad || !(d[k] >= lo[k] - slack && d[k] <= hi[k] + slack);
            }
            const PixTaps t = field_taps(W, H, X - d[0], Y - d[1]);
            if (t.inside) {
                for (int k = 0; k < 2; ++k)
                    bad = bad || t.x[k] < 0 || t.x[k] >= W || t.y[k] < 0 || t.y[k] >= H || !(t.wx[k] >= 0.0 && t.wx[k] <= 1.0) ||
                          !(t.wy[k] >= 0.0 && t.wy[k] <= 1.0);
                if (!bad) {
                    const double a = field_sample(img, W, t), b = field_sample(img, W, t);
                    bad = std::memcmp(&a, &b, sizeof a) != 0 || (a == a && !(a >= 0.0 && a <= 1.0 + 1e-12));
                    ++samples;
                }
            }
            if (bad) {
                std::printf("FAIL it %ld: pixel (%g, %g) displacement (%g, %g) taps x %d %d y %d %d in %d x %d\n", it, X, Y, d[0],
                            d[1], t.x[0], t.x[1], t.y[0], t.y[1], W, H);
                ++failures;
                break;
            }
        }
        std::free(img);
        std::free(v);
        std::free(u);
        std::free(xs);
        std::free(ys);
    }
    if (failures) return 1;
    std::printf("ok: %ld iterations, %ld samples taken\n", iters, samples);
    return 0;
}
