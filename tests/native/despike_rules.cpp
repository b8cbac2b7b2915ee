// The plan of the median/MAD despiking (csrc/despike_plan.hpp) on the host, under sanitizers.  What is checked is stated
// here on its own, not taken from the plan:
//   * parameters: every refusal with its code, the requests either side of each limit -- radius 0, 1, 3, 4; n_iter 0, 1, 8,
//     9; nsigma 0, -1, NaN, +Inf, the smallest positive number; floor -1e-300, -0.0, 0, NaN, +Inf; min_neighbours 0, 1,
//     (2R+1)^2 - 1 and one more for every R; sign and replace -1, 0, 1, 2; a null pointer; shapes of 0 rows or columns and of
//     2^31 - 1 and 2^31 pixels;
//   * geometry: for the shapes 1x1, 1x300, 300x1, 5x5 and one pixel past and one short of a tile in each axis, with
//     R = 1, 2, 3, the launch -- every workgroup looping over its work items, every thread of it -- owns every pixel exactly
//     once and nothing outside the image; what an item stages (the tile and its halo) and every neighbour a thread reads lie
//     inside the LDS bytes the plan gives; the same with the launch held to 1, 2 and 7 workgroups;
//   * the decision: despike_decide, the function the kernel calls, against a brute-force sort on seeded neighbourhoods with
//     ties, NaN slots and every k from 0 to 48 (and 0 to 8, 0 to 24 for the smaller windows), bit for bit, for either sign,
//     with and without a floor.
// Host compiler only; prints "ok: ..." and returns 0, or says what differs.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../euispice_coreg_amd/csrc/despike_plan.hpp"

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

bool taken(const coreg_despike_params& p) {
    const bool a = despike_params_refusal(&p) == nullptr;
    const DespikePlan pl = despike_plan(5, 5, &p);  // the plan says the same, a refusal with COREG_EINVAL and a message
    CHECK(a ? (pl.code == COREG_OK && pl.msg == nullptr) : (pl.code == COREG_EINVAL && pl.msg != nullptr), "plan and refusal disagree");
    return a;
}

void check_params() {
    CHECK(taken(good()), "the defaults were refused");
    CHECK(despike_params_refusal(nullptr) != nullptr && despike_plan(5, 5, nullptr).code == COREG_EINVAL, "null parameters were taken");
    struct IntCase {
        int32_t coreg_despike_params::*field;
        const char* name;
        int value;
        bool ok;
    };
    const IntCase ints[] = {
        {&coreg_despike_params::radius, "radius", 0, false},   {&coreg_despike_params::radius, "radius", 1, true},
        {&coreg_despike_params::radius, "radius", 3, true},    {&coreg_despike_params::radius, "radius", 4, false},
        {&coreg_despike_params::radius, "radius", -1, false},  {&coreg_despike_params::n_iter, "n_iter", 0, false},
        {&coreg_despike_params::n_iter, "n_iter", 1, true},    {&coreg_despike_params::n_iter, "n_iter", 8, true},
        {&coreg_despike_params::n_iter, "n_iter", 9, false},   {&coreg_despike_params::sign, "sign", -1, false},
        {&coreg_despike_params::sign, "sign", 0, true},        {&coreg_despike_params::sign, "sign", 1, true},
        {&coreg_despike_params::sign, "sign", 2, false},       {&coreg_despike_params::replace, "replace", -1, false},
        {&coreg_despike_params::replace, "replace", 0, true},  {&coreg_despike_params::replace, "replace", 1, true},
        {&coreg_despike_params::replace, "replace", 2, false},
    };
    for (const IntCase& c : ints) {
        coreg_despike_params p = good();
        if (c.field == &coreg_despike_params::radius) p.min_neighbours = 1;  // (good for every radius)
        p.*(c.field) = c.value;
        CHECK(taken(p) == c.ok, "%s = %d: %s", c.name, c.value, c.ok ? "refused" : "taken");
    }
    for (int R = 1; R <= 3; ++R) {
        const int most = (2 * R + 1) * (2 * R + 1) - 1;
        CHECK(despike_neighbours(R) == most, "neighbours of R = %d", R);
        for (int m : {0, 1, most, most + 1, -3}) {
            coreg_despike_params p = good();
            p.radius = R;
            p.min_neighbours = m;
            CHECK(taken(p) == (m >= 1 && m <= most), "R = %d, min_neighbours = %d", R, m);
        }
    }
    struct DblCase {
        double value;
        bool ok;
    };
    for (const DblCase& c : {DblCase{0.0, false}, {-0.0, false}, {-1.0, false}, {kNaN, false}, {kInf, false}, {-kInf, false}, {5e-324, true}, {1e300, true}}) {
        coreg_despike_params p = good();
        p.nsigma = c.value;
        CHECK(taken(p) == c.ok, "nsigma = %g", c.value);
    }
    for (const DblCase& c : {DblCase{0.0, true}, {-0.0, true}, {-1e-300, false}, {-1.0, false}, {kNaN, false}, {kInf, false}, {-kInf, false}, {1e300, true}}) {
        coreg_despike_params p = good();
        p.floor = c.value;
        CHECK(taken(p) == c.ok, "floor = %g", c.value);
    }
    // shapes
    const coreg_despike_params p = good();
    CHECK(despike_plan(0, 5, &p).code == COREG_EINVAL, "0 rows");
    CHECK(despike_plan(5, 0, &p).code == COREG_EINVAL, "0 columns");
    CHECK(despike_plan(-1, -1, &p).code == COREG_EINVAL, "negative shape");
    CHECK(despike_plan(1, 2147483647ll, &p).code == COREG_OK, "2^31 - 1 pixels");
    CHECK(despike_plan(2147483647ll, 1, &p).code == COREG_OK, "2^31 - 1 pixels, one column");
    CHECK(despike_plan(2, 1073741824ll, &p).code == COREG_EINVAL, "2^31 pixels");
    CHECK(despike_plan(46341, 46341, &p).code == COREG_EINVAL, "46341^2 pixels");
    CHECK(despike_plan(46340, 46340, &p).code == COREG_OK, "46340^2 pixels");
    CHECK(despike_plan(4000000000ll, 4000000000ll, &p).code == COREG_EINVAL, "a product past 2^63");
    // the parameters are looked at before the shape
    coreg_despike_params bad = good();
    bad.radius = 7;
    const DespikePlan both = despike_plan(0, 0, &bad);
    CHECK(both.code == COREG_EINVAL && both.msg && std::strstr(both.msg, "radius"), "the parameters are looked at first");
}

// one launch, simulated thread by thread; grid_cap > 0 holds the launch to that many workgroups
void check_geometry(int H, int W, int R, long long grid_cap) {
    coreg_despike_params prm = good();
    prm.radius = R;
    const DespikePlan p = despike_plan(H, W, &prm);
    CHECK(p.code == COREG_OK, "%dx%d R=%d: refused", H, W, R);
    if (p.code != COREG_OK) return;
    const DespikeGeom& g = p.g;
    CHECK(g.W == W && g.H == H && g.items == (long long)g.n_tx * g.n_ty, "%dx%d: geometry fields", H, W);
    CHECK(p.grid >= 1 && p.grid <= kDespikeMaxGrid && p.grid <= g.items, "%dx%d: grid", H, W);
    const long long staged = (long long)(kDespikeTileW + 2 * R) * (kDespikeTileH + 2 * R);  // float64 entries of an item
    CHECK(p.lds == (size_t)staged * sizeof(double) && p.lds <= 8 * 1024 && despike_lds_entries(R) == staged, "%dx%d R=%d: LDS %zu", H, W, R, p.lds);
    std::vector<int> hits((size_t)H * W, 0);
    int outside = 0, lds_over = 0, wrong_nb = 0;
    const long long grid = grid_cap > 0 ? std::min<long long>(grid_cap, p.grid) : p.grid;
    const int pitch = despike_lds_pitch(R);
    for (long long b = 0; b < grid; ++b)
        for (long long item = b; item < g.items; item += grid) {
            int y0, x0;
            despike_origin(g, item, &y0, &x0);
            if (y0 < 0 || y0 >= H || x0 < 0 || x0 >= W || y0 % kDespikeTileH || x0 % kDespikeTileW) ++outside;
            for (int t = 0; t < kDespikeThreads; ++t) {
                // what the thread reads, owner or not: entries of the staged window, each the pixel it stands for
                for (int dy = -R; dy <= R; ++dy)
                    for (int dx = -R; dx <= R; ++dx) {
                        const int e = despike_lds_index(R, t, dy, dx);
                        if (e < 0 || e >= staged || (size_t)(e + 1) * sizeof(double) > p.lds) ++lds_over;
                        const long long y = (long long)y0 - R + e / pitch, x = (long long)x0 - R + e % pitch;
                        if (y != (long long)y0 + t / kDespikeTileW + dy || x != (long long)x0 + t % kDespikeTileW + dx) ++wrong_nb;
                    }
                int row, col;
                if (!despike_pixel(g, item, t, &row, &col)) {
                    if (row < H && col < W) ++outside;  // (not owned: one coordinate is past its end)
                    continue;
                }
                if (row < 0 || row >= H || col < 0 || col >= W || row != y0 + t / kDespikeTileW || col != x0 + t % kDespikeTileW) ++outside;
                else ++hits[(size_t)row * W + col];
            }
        }
    int wrong = 0;
    for (int v : hits) wrong += v != 1;
    CHECK(wrong == 0 && outside == 0 && lds_over == 0 && wrong_nb == 0,
          "%dx%d R=%d grid %lld: %d pixels not once, %d outside, %d LDS, %d neighbours misplaced", H, W, R, grid, wrong, outside,
          lds_over, wrong_nb);
}

// ---- the decision against a brute-force sort ----------------------------------------------------------------------------
unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
unsigned next_u32() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(rng_state >> 33);
}
double next_unit() { return (next_u32() % 1000001u) / 1000000.0; }

double middle(std::vector<double> s) {
    std::sort(s.begin(), s.end());
    const size_t k = s.size();
    if (k % 2) return s[k / 2];
    volatile double sum = s[k / 2 - 1] + s[k / 2];  // (rounded on its own)
    return sum * 0.5;
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

template <int NN>
void check_decisions(int rounds) {
    int bad_flag = 0, bad_med = 0, n_flag = 0, n_keep = 0;
    for (int k = 0; k <= NN; ++k)
        for (int round = 0; round < rounds; ++round) {
            // k finite values in seeded slots of the NN, NaN elsewhere; kinds: integers with many ties, all equal, noise
            double n[NN];
            for (int i = 0; i < NN; ++i) n[i] = kNaN;
            const int kind = round % 4;
            std::vector<double> vals;
            int placed = 0;
            while (placed < k) {
                const int slot = (int)(next_u32() % NN);
                if (n[slot] == n[slot]) continue;
                double v;
                if (kind == 0) v = (double)(next_u32() % 4);              // ties everywhere
                else if (kind == 1) v = 7.0;                              // a flat neighbourhood: mad = 0
                else if (kind == 2) v = 100.0 + 10.0 * next_unit();       // noise
                else v = (next_u32() % 3 ? 50.0 : 50.0 + 1e-9 * (double)(next_u32() % 5)) - 50.0 * (next_u32() % 2);  // two clusters
                n[slot] = v;
                vals.push_back(v);
                ++placed;
            }
            coreg_despike_params p = good();
            p.radius = NN == 8 ? 1 : NN == 24 ? 2 : 3;
            p.min_neighbours = 1 + (int)(next_u32() % NN);
            p.sign = (int)(next_u32() % 2);
            p.floor = round % 3 == 0 ? 0.5 : 0.0;
            p.nsigma = round % 5 == 0 ? 1.0 : 5.0;
            const double c = kind == 2 ? 100.0 + 60.0 * next_unit() : -3.0 + (double)(next_u32() % 12);
            // the rule, by sorting
            bool want = false;
            double want_med = 0.0;
            if (k >= p.min_neighbours) {
                want_med = middle(vals);
                std::vector<double> dev;
                for (double v : vals) {
                    volatile double d = v - want_med;
                    dev.push_back(std::fabs(d));
                }
                const double mad = middle(dev);
                volatile double s = 1.4826 * mad;
                const double scale = s > p.floor ? (double)s : p.floor;
                volatile double d = c - want_med;
                volatile double lim = p.nsigma * scale;
                want = scale > 0.0 && (p.sign == COREG_DESPIKE_BOTH ? std::fabs(d) > lim : d > lim);
            }
            const DespikeDecision got = despike_decide<NN>(c, n, p);
            bad_flag += got.flagged != want;
            bad_med += !same_bits(got.med, want_med);
            (want ? n_flag : n_keep)++;
        }
    CHECK(bad_flag == 0 && bad_med == 0, "decision over %d slots: %d flags and %d medians differ from the sort", NN, bad_flag, bad_med);
    CHECK(n_flag > rounds && n_keep > rounds, "decision over %d slots: the cases decide both ways (%d flagged, %d kept)", NN, n_flag, n_keep);
}
}  // namespace

int main() {
    check_params();
    const int TH = kDespikeTileH, TW = kDespikeTileW;
    const int shapes[][2] = {{1, 1}, {1, 300}, {300, 1}, {5, 5}, {TH + 1, TW + 1}, {TH - 1, TW - 1}, {TH, TW}, {2 * TH + 1, TW - 1}, {TH - 1, 3 * TW + 1}};
    for (const auto& s : shapes)
        for (int R = 1; R <= 3; ++R)
            for (long long cap : {0ll, 1ll, 2ll, 7ll}) check_geometry(s[0], s[1], R, cap);
    // the 32 lanes an LDS read serves together read 32 neighbouring entries of one staged row
    for (int R = 1; R <= 3; ++R)
        CHECK(despike_lds_index(R, 31, 0, 0) - despike_lds_index(R, 0, 0, 0) == 31 && despike_lds_index(R, 63, 0, 0) - despike_lds_index(R, 32, 0, 0) == 31,
              "a 32-lane group reads one staged row");
    // a row / a column of 2^31 - 1 pixels: the last work item's last threads (no coordinate sum may overflow: UBSan)
    {
        const coreg_despike_params prm = good();
        const long long big = 2147483647ll;
        const DespikePlan pw = despike_plan(1, big, &prm), ph = despike_plan(big, 1, &prm);
        int row, col;
        const int last_col = (int)((big - 1) % TW), last_row = (int)((big - 1) % TH);
        CHECK(despike_pixel(pw.g, pw.g.items - 1, last_col, &row, &col) && row == 0 && col == big - 1, "last pixel of a long row");
        CHECK(!despike_pixel(pw.g, pw.g.items - 1, last_col + 1, &row, &col) && col == big, "past the end of a long row");
        CHECK(despike_pixel(ph.g, ph.g.items - 1, last_row * TW, &row, &col) && row == big - 1 && col == 0, "last pixel of a long column");
        CHECK(!despike_pixel(ph.g, ph.g.items - 1, (last_row + 1) * TW, &row, &col) && row == big, "past the end of a long column");
        CHECK(pw.grid == kDespikeMaxGrid && ph.grid == kDespikeMaxGrid, "a long image: the grid cap");
    }
    check_decisions<8>(200);
    check_decisions<24>(120);
    check_decisions<48>(80);
    if (n_bad) {
        std::printf("%d of %d checks failed\n", n_bad, n_checked);
        return 1;
    }
    std::printf("ok: despike rules (%d checks)\n", n_checked);
    return 0;
}
