// The planner of the NaN-aware smoothing (csrc/smooth_plan.hpp) on the host, under sanitizers.  What is checked is stated
// here on its own, not taken from the planner:
//   * tables: every refusal with its code, the requests either side of each limit -- 0, 1, 2, 127, 128, 129, 130, 131
//     entries; an entry NaN, +Inf, -Inf, negative, -0.0 (good: not below zero); a sum of zero against one positive entry; a
//     null pointer; the y table is looked at before the x table; shapes of 0 rows or columns and of 2^31 - 1 and 2^31 pixels;
//   * geometry: for the shapes 1x1, 1x300, 300x1, 257x3, 5x5 (and 3x257, 130x70) with r = 0, 1, 8, 64 on either axis the
//     row pass -- every workgroup of the launch looping over its work items, every thread of it -- writes every pixel exactly
//     once and nothing outside the image, and so does the column pass with its four turns per thread; what a work item stages
//     in LDS (the segment or tile and its halo) fits the bytes the plan asks for, and those stay at or under 48 KiB;
//   * the same with the launch held to 1, 2 and 7 workgroups (the grid-stride loops, as an image of more than 65536 work
//     items runs them).
// Host compiler only; prints "ok: ..." and returns 0, or says what differs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../euispice_coreg_amd/csrc/smooth_plan.hpp"

using namespace coreg;

namespace {
int n_bad = 0, n_checked = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        ++n_checked;                           \
        if (!(cond)) {                         \
            ++n_bad;                           \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");                 \
        }                                      \
    } while (0)

std::vector<double> flat(int n, double v = 1.0) { return std::vector<double>((size_t)(n > 0 ? n : 0), v); }

void check_tables() {
    const double one[1] = {1.0};
    for (int n : {0, 2, 128, 130, 131, 4, 1000}) {
        const std::vector<double> t = flat(n);
        const double* p = t.empty() ? one : t.data();
        CHECK(smooth_table_refusal(p, n) != nullptr, "a table of %d entries was taken", n);
        CHECK(smooth_plan(5, 5, p, n, one, 1).code == COREG_EINVAL, "wy of %d entries: no COREG_EINVAL", n);
        CHECK(smooth_plan(5, 5, one, 1, p, n).code == COREG_EINVAL, "wx of %d entries: no COREG_EINVAL", n);
    }
    CHECK(smooth_table_refusal(one, -1) != nullptr, "a table of -1 entries was taken");
    for (int n : {1, 3, 127, 129}) {
        const std::vector<double> t = flat(n);
        CHECK(smooth_table_refusal(t.data(), n) == nullptr, "a table of %d entries was refused", n);
        const SmoothPlan p = smooth_plan(5, 5, t.data(), n, one, 1);
        CHECK(p.code == COREG_OK && p.msg == nullptr && p.g.ry == n / 2 && p.g.rx == 0, "wy of %d entries: plan", n);
    }
    CHECK(smooth_table_refusal(nullptr, 1) != nullptr, "a null table was taken");
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (double bad : {nan, inf, -inf, -1e-300, -1.0}) {
        for (int at = 0; at < 3; ++at) {
            double t[3] = {0.25, 0.5, 0.25};
            t[at] = bad;
            CHECK(smooth_table_refusal(t, 3) != nullptr, "the entry %g at %d was taken", bad, at);
            CHECK(smooth_plan(4, 4, one, 1, t, 3).code == COREG_EINVAL, "the entry %g at %d: no COREG_EINVAL", bad, at);
        }
    }
    const double negzero[3] = {-0.0, 1.0, 0.0};
    CHECK(smooth_table_refusal(negzero, 3) == nullptr, "-0.0 is not below zero");
    const double zeros[3] = {0.0, 0.0, 0.0}, tiny[3] = {0.0, 0.0, 5e-324}, edge_only[3] = {1.0, 0.0, 0.0};
    CHECK(smooth_table_refusal(zeros, 3) != nullptr, "a table of zeros was taken");
    CHECK(smooth_table_refusal(tiny, 3) == nullptr, "one positive entry is a positive sum");
    CHECK(smooth_table_refusal(edge_only, 3) == nullptr, "a zero centre weight is allowed");
    const double huge[3] = {1.5e308, 1.5e308, 0.0};
    CHECK(smooth_table_refusal(huge, 3) != nullptr, "a sum that overflows was taken");
    // order: the y table first
    const SmoothPlan both = smooth_plan(4, 4, zeros, 3, flat(2).data(), 2);
    CHECK(both.code == COREG_EINVAL && both.msg && std::strstr(both.msg, "sum"), "the y table is looked at first");
    // shapes
    CHECK(smooth_plan(0, 5, one, 1, one, 1).code == COREG_EINVAL, "0 rows");
    CHECK(smooth_plan(5, 0, one, 1, one, 1).code == COREG_EINVAL, "0 columns");
    CHECK(smooth_plan(-1, -1, one, 1, one, 1).code == COREG_EINVAL, "negative shape");
    CHECK(smooth_plan(1, 2147483647ll, one, 1, one, 1).code == COREG_OK, "2^31 - 1 pixels");
    CHECK(smooth_plan(2147483647ll, 1, one, 1, one, 1).code == COREG_OK, "2^31 - 1 pixels, one column");
    CHECK(smooth_plan(2, 1073741824ll, one, 1, one, 1).code == COREG_EINVAL, "2^31 pixels");
    CHECK(smooth_plan(46341, 46341, one, 1, one, 1).code == COREG_EINVAL, "46341^2 pixels");
    CHECK(smooth_plan(46340, 46340, one, 1, one, 1).code == COREG_OK, "46340^2 pixels");
}

// one launch of both passes, simulated thread by thread; grid_cap > 0 holds the launch to that many workgroups
void check_geometry(int H, int W, int ry, int rx, long long grid_cap) {
    const std::vector<double> ty = flat(2 * ry + 1), tx = flat(2 * rx + 1);
    const SmoothPlan p = smooth_plan(H, W, ty.data(), 2 * ry + 1, tx.data(), 2 * rx + 1);
    CHECK(p.code == COREG_OK, "%dx%d r=(%d,%d): refused", H, W, ry, rx);
    if (p.code != COREG_OK) return;
    const SmoothGeom& g = p.g;
    CHECK(g.W == W && g.H == H && g.rx == rx && g.ry == ry, "%dx%d: geometry fields", H, W);
    CHECK(p.row_grid >= 1 && p.row_grid <= kSmoothMaxGrid && p.col_grid >= 1 && p.col_grid <= kSmoothMaxGrid, "%dx%d: grid", H, W);
    CHECK(p.col_lds == (size_t)2 * (kSmoothColH + 2 * ry) * kSmoothColW * sizeof(double) && p.col_lds <= 48 * 1024,
          "%dx%d ry=%d: column LDS %zu", H, W, ry, p.col_lds);
    CHECK(smooth_row_lds_bytes() >= (size_t)2 * (kSmoothSeg + 2 * rx) * sizeof(double) && smooth_row_lds_bytes() <= 8 * 1024,
          "row LDS");
    std::vector<int> hits((size_t)H * W, 0);
    int outside = 0, lds_over = 0;
    // row pass
    const long long row_grid = grid_cap > 0 ? std::min<long long>(grid_cap, p.row_grid) : p.row_grid;
    for (long long b = 0; b < row_grid; ++b)
        for (long long item = b; item < g.row_items; item += row_grid) {
            const int x0 = smooth_row_x0(g, item);
            for (int t = 0; t < kSmoothThreads; ++t) {
                int row, col;
                const bool live = smooth_row_pixel(g, item, t, &row, &col);
                if (row < 0 || row >= H) ++outside;  // (the row is staged by every thread, live or not)
                if (!live) continue;
                if (col < 0 || col >= W || col != x0 + t) ++outside;
                else ++hits[(size_t)row * W + col];
                // the taps thread t reads: z[t .. t + 2 rx] of kSmoothSeg + 2 rx staged entries
                if (t + 2 * rx >= kSmoothSeg + 2 * rx || (size_t)(kSmoothSeg + 2 * rx) * 2 * sizeof(double) > smooth_row_lds_bytes())
                    ++lds_over;
            }
        }
    int wrong = 0;
    for (int& v : hits) {
        wrong += v != 1;
        v = 0;
    }
    CHECK(wrong == 0 && outside == 0 && lds_over == 0, "%dx%d r=(%d,%d) grid %lld: row pass: %d pixels not once, %d outside, %d LDS",
          H, W, ry, rx, row_grid, wrong, outside, lds_over);
    // column pass
    outside = lds_over = 0;
    const long long col_grid = grid_cap > 0 ? std::min<long long>(grid_cap, p.col_grid) : p.col_grid;
    const long long staged = (long long)(kSmoothColH + 2 * ry) * kSmoothColW;  // doubles per plane
    for (long long b = 0; b < col_grid; ++b)
        for (long long item = b; item < g.col_items; item += col_grid) {
            int y0, x0;
            smooth_col_origin(g, item, &y0, &x0);
            if (y0 < 0 || y0 >= H || x0 < 0 || x0 >= W) ++outside;
            for (int t = 0; t < kSmoothThreads; ++t)
                for (int q = 0; q < kSmoothColQ; ++q) {
                    int row, col;
                    const int j = smooth_col_tile_row(t, q);
                    if (j < 0 || j >= kSmoothColH) ++lds_over;
                    // the last tap thread t reads: row j + 2 ry of the staged rows, column t % 16
                    if ((long long)(j + 2 * ry) * kSmoothColW + t % kSmoothColW >= staged || (size_t)staged * 2 * sizeof(double) > p.col_lds)
                        ++lds_over;
                    if (!smooth_col_pixel(g, item, t, q, &row, &col)) continue;
                    if (row < 0 || row >= H || col < 0 || col >= W || row != y0 + j || col != x0 + t % kSmoothColW) ++outside;
                    else ++hits[(size_t)row * W + col];
                }
        }
    wrong = 0;
    for (int v : hits) wrong += v != 1;
    CHECK(wrong == 0 && outside == 0 && lds_over == 0, "%dx%d r=(%d,%d) grid %lld: column pass: %d pixels not once, %d outside, %d LDS",
          H, W, ry, rx, col_grid, wrong, outside, lds_over);
}
}  // namespace

int main() {
    check_tables();
    const int shapes[][2] = {{1, 1}, {1, 300}, {300, 1}, {257, 3}, {5, 5}, {3, 257}, {130, 70}};
    const int reach[] = {0, 1, 8, 64};
    for (const auto& s : shapes)
        for (int ry : reach)
            for (int rx : reach)
                for (long long cap : {0ll, 1ll, 2ll, 7ll}) check_geometry(s[0], s[1], ry, rx, cap);
    // every thread of a wave's 32-lane LDS group reads two neighbouring staged rows: tile rows t / 16 of threads 0..31
    for (int q = 0; q < kSmoothColQ; ++q)
        CHECK(smooth_col_tile_row(31, q) - smooth_col_tile_row(0, q) == 1, "a 32-lane group spans two neighbouring rows");
    // a row / a column of 2^31 - 1 pixels: the last work item's last threads (no coordinate sum may overflow: UBSan)
    {
        const double one[1] = {1.0};
        const long long big = 2147483647ll;
        const SmoothPlan pw = smooth_plan(1, big, one, 1, one, 1), ph = smooth_plan(big, 1, one, 1, one, 1);
        int row, col;
        CHECK(smooth_row_pixel(pw.g, pw.g.row_items - 1, 254, &row, &col) && row == 0 && col == big - 1, "last pixel of a long row");
        CHECK(!smooth_row_pixel(pw.g, pw.g.row_items - 1, 255, &row, &col) && col == big, "past the end of a long row");
        CHECK(!smooth_col_pixel(pw.g, pw.g.col_items - 1, 15, 0, &row, &col), "past the end of a long row, column pass");
        CHECK(smooth_col_pixel(pw.g, pw.g.col_items - 1, 14, 0, &row, &col) && col == big - 1, "last pixel, column pass");
        CHECK(smooth_col_pixel(ph.g, ph.g.col_items - 1, 16 * 14, 3, &row, &col) && row == big - 1, "last pixel of a long column");
        CHECK(!smooth_col_pixel(ph.g, ph.g.col_items - 1, 16 * 15, 3, &row, &col) && row == big, "past the end of a long column");
    }
    if (n_bad) {
        std::printf("%d of %d checks failed\n", n_bad, n_checked);
        return 1;
    }
    std::printf("ok: smooth rules (%d checks)\n", n_checked);
    return 0;
}
