// The plan of coreg_despike_sum_planes_be (csrc/despike_planes_plan.hpp) on the host, under sanitizers.  What is checked is
// stated here on its own, not taken from the plan:
//   * refusals, each COREG_EINVAL with a message: a bad rule (the rule is looked at first); BITPIX 32, 16, 0, -16; H or W of
//     0 or below and 2^31 pixels; plane_stride one below H x W; n_sel -1 and 4097; base, out_sum and (n_sel > 0) plane_index
//     null; a negative plane index.  Taken: BITPIX -32 and -64, 2^31 - 1 pixels, plane_stride = H x W and above, n_sel 0, 1
//     and 4096, plane_index null with n_sel = 0, duplicates and any order;
//   * n_sel = 0: a plan with no plane and no work item of a pass;
//   * geometry, for the shapes 1x1, 1x40, 40x1, 5x7 and one pixel past a tile in each axis, 1, 3 and 6 planes, R = 1, 2, 3,
//     the launches held to 1, 2, 7 workgroups and not at all: a pass before the last -- every workgroup looping over its
//     (plane, tile) pairs, every thread of it -- owns every pixel of every plane exactly once and nothing else; the last
//     pass -- every workgroup looping over its tiles and, inside, over the planes in order -- likewise, and the planes of a
//     pixel come in increasing order; the window entries the threads stage per plane (entries t, t + 256, ...) cover the
//     window exactly once inside the LDS the plan gives for two windows;
//   * the sum: despike_planes_add over the planes against a sum written here, bit for bit, with NaN, +-Inf, both infinities
//     at one pixel, all-NaN pixels and no plane at all.
// Host compiler only; prints "ok: ..." and returns 0, or says what differs.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../euispice_coreg_amd/csrc/despike_planes_plan.hpp"

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

const double kInf = std::numeric_limits<double>::infinity(), kNaN = std::numeric_limits<double>::quiet_NaN();

coreg_despike_params good() {
    coreg_despike_params p;
    std::memset(&p, 0, sizeof(p));
    p.radius = 2;
    p.n_iter = 2;
    p.min_neighbours = 5;
    p.sign = COREG_DESPIKE_POSITIVE;
    p.replace = COREG_DESPIKE_NAN;
    p.nsigma = 5.0;
    p.floor = 0.0;
    return p;
}

bool refused(const DespikePlanesPlan& p) { return p.code == COREG_EINVAL && p.msg != nullptr; }
bool taken(const DespikePlanesPlan& p) { return p.code == COREG_OK && p.msg == nullptr; }

void check_refusals() {
    const coreg_despike_params prm = good();
    float pixels[12] = {0};
    double out[12] = {0};
    const int64_t idx[3] = {2, 0, 2};  // out of order, with a duplicate
    const void* base = pixels;
    CHECK(taken(despike_planes_plan(base, -32, 4, 2, 2, idx, 3, &prm, out)), "a good call was refused");
    CHECK(taken(despike_planes_plan(base, -64, 4, 2, 2, idx, 3, &prm, out)), "BITPIX -64 was refused");
    for (int bitpix : {32, 16, 8, 0, -16, 64, -33}) CHECK(refused(despike_planes_plan(base, bitpix, 4, 2, 2, idx, 3, &prm, out)), "BITPIX %d was taken", bitpix);
    CHECK(refused(despike_planes_plan(base, -32, 4, 0, 2, idx, 3, &prm, out)), "0 rows");
    CHECK(refused(despike_planes_plan(base, -32, 4, 2, 0, idx, 3, &prm, out)), "0 columns");
    CHECK(refused(despike_planes_plan(base, -32, 4, -1, -4, idx, 3, &prm, out)), "negative shape");
    CHECK(taken(despike_planes_plan(base, -32, 2147483647ll, 1, 2147483647ll, idx, 3, &prm, out)), "2^31 - 1 pixels");
    CHECK(refused(despike_planes_plan(base, -32, 4294967296ll, 2, 1073741824ll, idx, 3, &prm, out)), "2^31 pixels");
    CHECK(refused(despike_planes_plan(base, -32, 3, 2, 2, idx, 3, &prm, out)), "plane_stride below H x W");
    CHECK(refused(despike_planes_plan(base, -32, -4, 2, 2, idx, 3, &prm, out)), "negative plane_stride");
    CHECK(taken(despike_planes_plan(base, -32, 5, 2, 2, idx, 3, &prm, out)), "plane_stride above H x W");
    CHECK(refused(despike_planes_plan(base, -32, 4, 2, 2, idx, -1, &prm, out)), "n_sel -1");
    CHECK(kDespikePlanesMaxSel == 4096, "the cap of n_sel");
    std::vector<int64_t> many(4097, 0);
    CHECK(taken(despike_planes_plan(base, -32, 4, 2, 2, many.data(), 4096, &prm, out)), "n_sel 4096");
    CHECK(refused(despike_planes_plan(base, -32, 4, 2, 2, many.data(), 4097, &prm, out)), "n_sel 4097");
    CHECK(refused(despike_planes_plan(nullptr, -32, 4, 2, 2, idx, 3, &prm, out)), "null base");
    CHECK(refused(despike_planes_plan(base, -32, 4, 2, 2, idx, 3, &prm, nullptr)), "null out_sum");
    CHECK(refused(despike_planes_plan(base, -32, 4, 2, 2, nullptr, 3, &prm, out)), "null plane_index");
    CHECK(refused(despike_planes_plan(base, -32, 4, 2, 2, idx, 3, nullptr, out)), "null parameters");
    const int64_t neg[2] = {1, -1};
    CHECK(refused(despike_planes_plan(base, -32, 4, 2, 2, neg, 2, &prm, out)), "a negative plane index");
    // the rule is looked at first
    coreg_despike_params bad = good();
    bad.radius = 7;
    const DespikePlanesPlan both = despike_planes_plan(base, 16, 4, 2, 2, idx, 3, &bad, out);
    CHECK(refused(both) && std::strstr(both.msg, "radius"), "the rule is looked at first");
    for (int n_iter : {0, 9}) {
        bad = good();
        bad.n_iter = n_iter;
        CHECK(refused(despike_planes_plan(base, -32, 4, 2, 2, idx, 3, &bad, out)), "n_iter %d", n_iter);
    }
    // no plane: nothing to launch
    const DespikePlanesPlan none = despike_planes_plan(base, -32, 4, 2, 2, nullptr, 0, &prm, out);
    CHECK(taken(none) && none.n_sel == 0 && none.pairs == 0 && none.grid_pairs == 0 && none.plane_px == 4, "n_sel 0");
}

void check_geometry(int H, int W, int n_sel, int R, long long cap) {
    coreg_despike_params prm = good();
    prm.radius = R;
    std::vector<int64_t> idx((size_t)n_sel, 0);
    double dummy = 0.0;
    const DespikePlanesPlan p = despike_planes_plan(&dummy, -64, (long long)H * W, H, W, idx.data(), n_sel, &prm, &dummy);
    CHECK(taken(p), "%dx%dx%d R=%d: refused", n_sel, H, W, R);
    if (!taken(p)) return;
    const DespikeGeom& g = p.g;
    CHECK(g.H == H && g.W == W && p.n_sel == n_sel && p.plane_px == (long long)H * W && p.pairs == g.items * n_sel, "%dx%dx%d: plan fields", n_sel, H, W);
    CHECK(p.grid_pairs >= 1 && p.grid_pairs <= kDespikeMaxGrid && p.grid_pairs <= p.pairs && p.grid_tiles >= 1 && p.grid_tiles <= g.items, "%dx%dx%d: grids", n_sel, H, W);
    const long long entries = (long long)(kDespikeTileW + 2 * R) * (kDespikeTileH + 2 * R);
    CHECK(p.lds == 2 * (size_t)entries * sizeof(double) && p.lds <= 16 * 1024, "%dx%dx%d R=%d: LDS %zu", n_sel, H, W, R, p.lds);
    // the staging slots of the threads cover a window exactly once
    std::vector<int> staged((size_t)entries, 0);
    int over = 0;
    for (int t = 0; t < kDespikeThreads; ++t)
        for (int s = 0; s < despike_planes_stage_slots(R); ++s) {
            const long long e = t + (long long)s * kDespikeThreads;
            if (e < entries) ++staged[(size_t)e];
            else if (e >= (long long)despike_planes_stage_slots(R) * kDespikeThreads) ++over;
        }
    int holes = 0;
    for (int v : staged) holes += v != 1;
    CHECK(holes == 0 && over == 0, "R=%d: %d window entries not staged once", R, holes);
    // a pass before the last: (plane, tile) pairs
    std::vector<int> hits((size_t)n_sel * H * W, 0);
    int outside = 0;
    long long grid = cap > 0 ? std::min<long long>(cap, p.grid_pairs) : p.grid_pairs;
    for (long long b = 0; b < grid; ++b)
        for (long long pair = b; pair < p.pairs; pair += grid) {
            int plane;
            long long tile;
            despike_planes_pair(g, pair, &plane, &tile);
            if (plane < 0 || plane >= n_sel || tile < 0 || tile >= g.items || plane * g.items + tile != pair) {
                ++outside;
                continue;
            }
            for (int t = 0; t < kDespikeThreads; ++t) {
                int row, col;
                if (!despike_pixel(g, tile, t, &row, &col)) continue;
                if (row < 0 || row >= H || col < 0 || col >= W) ++outside;
                else ++hits[((size_t)plane * H + row) * W + col];
            }
        }
    int wrong = 0;
    for (int v : hits) wrong += v != 1;
    CHECK(wrong == 0 && outside == 0, "%dx%dx%d R=%d grid %lld, pairs: %d pixels not once, %d outside", n_sel, H, W, R, grid, wrong, outside);
    // the last pass: tiles, and inside a tile the planes in order
    std::fill(hits.begin(), hits.end(), 0);
    std::vector<int> last_plane((size_t)H * W, -1);
    outside = 0;
    int disorder = 0;
    grid = cap > 0 ? std::min<long long>(cap, p.grid_tiles) : p.grid_tiles;
    for (long long b = 0; b < grid; ++b)
        for (long long tile = b; tile < g.items; tile += grid)
            for (int t = 0; t < kDespikeThreads; ++t) {
                int row, col;
                if (!despike_pixel(g, tile, t, &row, &col)) continue;
                if (row < 0 || row >= H || col < 0 || col >= W) {
                    ++outside;
                    continue;
                }
                for (int k = 0; k < p.n_sel; ++k) {
                    ++hits[((size_t)k * H + row) * W + col];
                    if (last_plane[(size_t)row * W + col] != k - 1) ++disorder;
                    last_plane[(size_t)row * W + col] = k;
                }
            }
    wrong = 0;
    for (int v : hits) wrong += v != 1;
    CHECK(wrong == 0 && outside == 0 && disorder == 0, "%dx%dx%d R=%d grid %lld, tiles: %d pixels not once, %d outside, %d planes out of order", n_sel, H, W,
          R, grid, wrong, outside, disorder);
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

void check_sum() {
    // pixels of five planes: plain values whose sum depends on the order, NaN in some planes, NaN in all, +Inf, both infinities
    const int n_px = 7, n_sel = 5;
    const double v[n_sel][n_px] = {{1e16, 0.1, kNaN, kNaN, 3.0, kInf, -0.0},
                                   {1.0, 0.2, 2.5, kNaN, kInf, 1.0, -0.0},
                                   {-1e16, 0.3, kNaN, kNaN, 4.0, -kInf, kNaN},
                                   {1.0, kNaN, 1e-300, kNaN, kNaN, 2.0, -0.0},
                                   {3.0, 0.7, -2.5, kNaN, 5.0, kNaN, -0.0}};
    for (int i = 0; i < n_px; ++i) {
        double got = 0.0;
        volatile double want = 0.0;  // (every addition rounded on its own, in the order of the planes)
        for (int k = 0; k < n_sel; ++k) {
            got = despike_planes_add(got, v[k][i]);
            if (!std::isnan(v[k][i])) want = want + v[k][i];
        }
        const double w = want;
        CHECK((std::isnan(w) && std::isnan(got)) || w == got, "sum of pixel %d: %a, wanted %a", i, got, w);
        if (i == 0) CHECK(got == 4.0, "pixel 0 in the order of the planes is 4 (5 in exact arithmetic), not %a", got);
    }
    double all_nan = 0.0;
    for (int k = 0; k < 3; ++k) all_nan = despike_planes_add(all_nan, kNaN);
    CHECK(same_bits(all_nan, 0.0), "a pixel that is NaN in every plane sums to +0.0");
    double both = despike_planes_add(despike_planes_add(0.0, kInf), -kInf);
    CHECK(std::isnan(both), "+Inf and -Inf at one pixel sum to NaN");
    CHECK(despike_planes_add(despike_planes_add(0.0, kNaN), kInf) == kInf, "+Inf passes through");
}
}  // namespace

int main() {
    check_refusals();
    const int TH = kDespikeTileH, TW = kDespikeTileW;
    const int shapes[][2] = {{1, 1}, {1, 40}, {40, 1}, {5, 7}, {TH + 1, TW + 1}, {2 * TH + 3, TW + 5}};
    for (const auto& s : shapes)
        for (int n_sel : {1, 3, 6})
            for (int R = 1; R <= 3; ++R)
                for (long long cap : {0ll, 1ll, 2ll, 7ll}) check_geometry(s[0], s[1], n_sel, R, cap);
    check_sum();
    if (n_bad) {
        std::printf("%d of %d checks failed\n", n_bad, n_checked);
        return 1;
    }
    std::printf("ok: despike planes rules (%d checks)\n", n_checked);
    return 0;
}
