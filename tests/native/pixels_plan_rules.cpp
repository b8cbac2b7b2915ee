// The planner of the pixel-lag sweep (csrc/pixels_plan.hpp) on the host, under sanitizers.  What is checked is stated
// here on its own, not taken from the planner:
//   * groups: for nine dx lists the groups cover the list in order, each index once, 1 to 16 entries, dx_min the smallest
//     of them, all within 16 columns, and every group but the last cannot take the next entry;
//   * windows: for every n <= 40, size <= n, step <= size the count is the smallest K >= 1 with (K - 1) step + size >= n,
//     and the last window begins inside the axis;
//   * band: cw = min(width, 2048), bh = max(1, min(64, 2048 / cw, height)) and the four bounds that keep a band within the
//     kernels' LDS, for whole images and for tiles of thirty shapes;
//   * blob: the sections of a plain, two mutual-information and an apodized plan lie in order, the doubles on multiples of
//     8 bytes, the total is the end of the last, and what the writer wrote reads back;
//   * refusals: one request per check with its code and message, the boundary pairs either side of each limit, and three
//     requests that break two checks at once (the first check in the order wins).
// Host compiler only; prints "ok: ..." and returns 0, or says what differs.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <limits>
#include <string>

#include "../../euispice_coreg_amd/csrc/pixels_plan.hpp"

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

// ---- groups ---------------------------------------------------------------------------------------------------------
void check_groups(const char* name, const std::vector<int32_t>& dx) {
    const int n = (int)dx.size();
    const std::vector<PixGroup> g = pixels_groups(dx.data(), n);
    int next = 0;
    for (size_t k = 0; k < g.size(); ++k) {
        CHECK(g[k].first == next, "%s: group %zu begins at %d, not %d", name, k, g[k].first, next);
        CHECK(g[k].count >= 1 && g[k].count <= 16, "%s: group %zu has %d entries", name, k, g[k].count);
        if (g[k].first != next || g[k].count < 1 || g[k].first + g[k].count > n) return;
        int lo = dx[next], hi = lo;
        for (int i = next; i < next + g[k].count; ++i) {
            lo = std::min(lo, dx[i]);
            hi = std::max(hi, dx[i]);
        }
        CHECK(g[k].dx_min == lo, "%s: group %zu dx_min %d, smallest entry %d", name, k, g[k].dx_min, lo);
        CHECK(hi - lo <= 15, "%s: group %zu spans %d columns", name, k, hi - lo);
        next += g[k].count;
        if (k + 1 < g.size()) {
            const int v = dx[next];
            CHECK(g[k].count == 16 || std::max(hi, v) - std::min(lo, v) > 15, "%s: group %zu could take entry %d", name, k, next);
        }
    }
    CHECK(next == n, "%s: the groups cover %d of %d entries", name, next, n);
}

std::vector<int32_t> run(int first, int n, int step) {
    std::vector<int32_t> v;
    for (int i = 0; i < n; ++i) v.push_back(first + i * step);
    return v;
}

void groups() {
    check_groups("[0]", {0});
    check_groups("16 consecutive", run(-8, 16, 1));
    check_groups("17 consecutive", run(-8, 17, 1));
    check_groups("[0, 15, 16]", {0, 15, 16});
    check_groups("[0, 16]", {0, 16});
    check_groups("20 descending", run(9, 20, -1));
    check_groups("[0, 15, -1]", {0, 15, -1});
    check_groups("[3, 3, 3]", {3, 3, 3});
    std::vector<int32_t> r;
    uint32_t s = 12345u;
    for (int i = 0; i < 100; ++i) {
        s = s * 1664525u + 1013904223u;
        r.push_back((int32_t)((s >> 8) % 81u) - 40);
    }
    check_groups("100 random", r);
    CHECK(pixels_groups(run(-8, 16, 1).data(), 16).size() == 1, "16 consecutive lags are not one group");
    const std::vector<int32_t> c17 = run(-8, 17, 1);
    const std::vector<PixGroup> g17 = pixels_groups(c17.data(), 17);
    CHECK(g17.size() == 2 && g17[0].count == 16 && g17[1].count == 1, "17 consecutive lags are not 16 + 1");
    const int32_t far[2] = {0, 16};
    CHECK(pixels_groups(far, 2).size() == 2, "[0, 16] is not two groups");
}

// ---- windows --------------------------------------------------------------------------------------------------------
void windows() {
    for (int n = 1; n <= 40; ++n)
        for (int size = 1; size <= n; ++size)
            for (int step = 1; step <= size; ++step) {
                long long K = 1;
                while ((K - 1) * step + size < n) ++K;
                const long long got = pixels_windows(n, size, step);
                CHECK(got == K, "windows(%d, %d, %d) = %lld, brute force %lld", n, size, step, got, K);
                CHECK((got - 1) * step < n, "windows(%d, %d, %d): the last window begins outside", n, size, step);
            }
}

// ---- a request ------------------------------------------------------------------------------------------------------
struct Req {
    std::vector<int32_t> dx = {-1, 0, 1}, dy = {0, 1};
    std::vector<double> rot = {0.0};
    coreg_pixels_plan pl = {};
    bool null_plan = false, null_out = false, null_dx = false;
    int method = COREG_METHOD_CORRELATION;
    bool tiled = false, stepped = false, weighted = false, only_wy = false;
    int32_t tile[2] = {4, 5}, step[2] = {4, 5};
    std::vector<double> wy, wx;
    PixHave have = {true, true, 20, 12, 0, 0};  // a small image of 12 rows x 20 columns
    double out = 0.0;
    Req() {
        pl.ratio1 = pl.ratio2 = 1.0;
        pl.sub_ny = 80;
        pl.sub_nx = 100;
        pl.l0 = pl.l1 = 10;
        pl.xc = 10;
        pl.yc = 6;
    }
    void apodize(int th, int tw) {
        tiled = weighted = true;
        tile[0] = step[0] = th;
        tile[1] = step[1] = tw;
        wy.assign((size_t)std::max(th, 1), 1.0);
        wx.assign((size_t)std::max(tw, 1), 1.0);
    }
    PixPlan plan() {
        pl.lag_dx = null_dx ? nullptr : dx.data();
        pl.lag_dy = dy.data();
        pl.lag_drot = rot.data();
        pl.n_dx = (int32_t)dx.size();
        pl.n_dy = (int32_t)dy.size();
        pl.n_rot = (int32_t)rot.size();
        const PixRequest rq = {null_plan ? nullptr : &pl, method, tiled ? tile : nullptr, stepped ? step : nullptr,
                               weighted ? wy.data() : nullptr, weighted && !only_wy ? wx.data() : nullptr, null_out ? nullptr : &out};
        return pixels_plan(rq, have);
    }
};
typedef std::function<void(Req&)> Change;

void accepted(const char* name, const Change& change) {
    Req r;
    change(r);
    const PixPlan p = r.plan();
    CHECK(p.code == COREG_OK, "%s: refused with %d \"%s\"", name, p.code, p.msg ? p.msg : "");
}
void refused(const char* name, const Change& change, int code, const char* msg) {
    Req r;
    change(r);
    const PixPlan p = r.plan();
    CHECK(p.code == code && p.msg && std::string(p.msg) == msg, "%s: got %d \"%s\", expected %d \"%s\"", name, p.code,
          p.msg ? p.msg : "(accepted)", code, msg);
}

// ---- band -----------------------------------------------------------------------------------------------------------
void band_of(const char* what, int width, int height, const PixPlan& p) {
    CHECK(p.code == COREG_OK, "band %s %d x %d: refused \"%s\"", what, width, height, p.msg ? p.msg : "");
    if (p.code != COREG_OK) return;
    const int cw = std::min(width, 2048), bh = std::max(1, std::min(std::min(64, 2048 / cw), height));
    CHECK(p.cw == cw && p.bh == bh, "band %s %d x %d: (%d, %d), expected (%d, %d)", what, width, height, p.cw, p.bh, cw, bh);
    CHECK(p.cw >= 1 && p.bh >= 1 && p.bh <= kPixBandRows, "band %s %d x %d: (%d, %d) out of range", what, width, height, p.cw, p.bh);
    CHECK(p.cw * p.bh <= kPixTile, "band %s %d x %d: %d pixels", what, width, height, p.cw * p.bh);
    CHECK(p.bh * (p.cw + kPixG - 1) <= kPixLdsB, "band %s %d x %d: %d box pixels", what, width, height, p.bh * (p.cw + kPixG - 1));
}
void bands() {
    for (int width : {1, 7, 2047, 2048, 2049, 5000})
        for (int height : {1, 63, 64, 65, 4000}) {
            Req whole, part;
            whole.have.w = width;
            whole.have.h = height;
            part.have.w = width + 3;
            part.have.h = height + 2;
            part.tiled = true;
            part.tile[0] = height;
            part.tile[1] = width;
            for (Req* r : {&whole, &part}) {
                r->pl.sub_ny = r->have.h + 40;
                r->pl.sub_nx = r->have.w + 40;
            }
            band_of("image", width, height, whole.plan());
            band_of("tile", width, height, part.plan());
        }
}

// ---- blob -----------------------------------------------------------------------------------------------------------
void blob_of(const char* name, Req& r, const std::vector<double>& a, const std::vector<double>& b) {
    const PixPlan p = r.plan();
    CHECK(p.code == COREG_OK, "blob %s: refused \"%s\"", name, p.msg ? p.msg : "");
    if (p.code != COREG_OK) return;
    const size_t n_dx = r.dx.size(), n_dy = r.dy.size();
    CHECK(p.off_dx == p.groups.size() * sizeof(PixGroup) && p.off_dx + n_dx * 4 <= p.off_dy, "blob %s: dx section", name);
    CHECK(p.off_dy % 4 == 0 && p.off_dx % 4 == 0, "blob %s: int sections not on 4 bytes", name);
    CHECK((p.off_dy + n_dy * 4) % 8 != 0, "blob %s: the int sections were meant to end off an 8-byte boundary", name);
    CHECK((size_t)p.n_a == a.size() && (size_t)p.n_b == b.size(), "blob %s: %d + %d doubles", name, p.n_a, p.n_b);
    size_t end = p.off_dy + n_dy * 4;
    if (!a.empty()) {
        CHECK(p.off_a >= end && p.off_a % 8 == 0, "blob %s: first double section at %zu", name, p.off_a);
        CHECK(p.off_b >= p.off_a + a.size() * 8 && p.off_b % 8 == 0, "blob %s: second double section at %zu", name, p.off_b);
        end = p.off_b + b.size() * 8;
    }
    CHECK(p.bytes == end, "blob %s: %zu bytes, the last section ends at %zu", name, p.bytes, end);
    std::vector<unsigned char> blob(p.bytes, (unsigned char)0xAB);
    pixels_plan_write(p, &r.pl, a.empty() ? nullptr : a.data(), b.empty() ? nullptr : b.data(), blob.data());
    const PixGroup* g = pixels_plan_at<PixGroup>(blob.data(), 0);
    for (size_t k = 0; k < p.groups.size(); ++k)
        CHECK(g[k].first == p.groups[k].first && g[k].count == p.groups[k].count && g[k].dx_min == p.groups[k].dx_min,
              "blob %s: group %zu reads back differently", name, k);
    for (size_t i = 0; i < n_dx; ++i) CHECK(pixels_plan_at<int>(blob.data(), p.off_dx)[i] == r.dx[i], "blob %s: dx[%zu]", name, i);
    for (size_t j = 0; j < n_dy; ++j) CHECK(pixels_plan_at<int>(blob.data(), p.off_dy)[j] == r.dy[j], "blob %s: dy[%zu]", name, j);
    for (size_t k = 0; k < a.size(); ++k) CHECK(pixels_plan_at<double>(blob.data(), p.off_a)[k] == a[k], "blob %s: a[%zu]", name, k);
    for (size_t k = 0; k < b.size(); ++k) CHECK(pixels_plan_at<double>(blob.data(), p.off_b)[k] == b[k], "blob %s: b[%zu]", name, k);
}
void blobs() {
    std::vector<double> e3, e31, wy, wx;
    for (int k = 0; k < 31; ++k) e31.push_back(0.5 * k - 3.0);
    e3.assign(e31.begin(), e31.begin() + 3);
    for (int k = 0; k < 5; ++k) wy.push_back(0.25 + k);
    for (int k = 0; k < 7; ++k) wx.push_back(7.5 - k);
    Req plain, mi_a, mi_b, lct;
    blob_of("plain", plain, {}, {});
    mi_a.method = mi_b.method = COREG_METHOD_MUTUAL_INFORMATION;
    mi_a.have.n_edges_small = 3;
    mi_a.have.n_edges_large = 31;
    blob_of("mutual information 3 / 31", mi_a, e3, e31);
    mi_b.have.n_edges_small = 31;
    mi_b.have.n_edges_large = 3;
    blob_of("mutual information 31 / 3", mi_b, e31, e3);
    lct.apodize(5, 7);
    lct.wy = wy;
    lct.wx = wx;
    blob_of("apodized 5 x 7", lct, wy, wx);
}

// ---- refusals -------------------------------------------------------------------------------------------------------
const char* kShift = "too large shift : outside FSI";
const char* kWeight = "pixels: a weight is negative or not finite";
const char* kStep = "pixels: the tile step must lie within [1, tile rows] x [1, tile columns]";
const char* kCorrOnly = "pixels: weight tables belong to the correlation (no weighted residus_masked or histogram)";
const char* kBins = "pixels: mutual information needs its bins (coreg_pixels_set_bins)";

void refusals() {
    // one per check, in the order of the checks
    refused("residus", [](Req& r) { r.method = COREG_METHOD_RESIDUS; }, COREG_ENOTIMPL,
            "pixels: method residus is not implemented (the reference's pxlshift has no such score); residus_masked is");
    refused("method 7", [](Req& r) { r.method = 7; }, COREG_EINVAL, "pixels: unknown method");
    refused("one weight table", [](Req& r) { r.apodize(4, 5); r.only_wy = true; }, COREG_EINVAL,
            "pixels: an apodized sweep needs both weight tables and a tile");
    refused("weight tables, no tile", [](Req& r) { r.apodize(4, 5); r.tiled = false; }, COREG_EINVAL,
            "pixels: an apodized sweep needs both weight tables and a tile");
    refused("weighted residus_masked", [](Req& r) { r.apodize(4, 5); r.method = COREG_METHOD_RESIDUS_MASKED; }, COREG_EINVAL, kCorrOnly);
    refused("weighted histogram", [](Req& r) { r.apodize(4, 5); r.method = COREG_METHOD_MUTUAL_INFORMATION; r.have.n_edges_small = r.have.n_edges_large = 4; },
            COREG_EINVAL, kCorrOnly);
    refused("no bins", [](Req& r) { r.method = COREG_METHOD_MUTUAL_INFORMATION; }, COREG_ESTATE, kBins);
    refused("one edge list", [](Req& r) { r.method = COREG_METHOD_MUTUAL_INFORMATION; r.have.n_edges_small = 4; }, COREG_ESTATE, kBins);
    refused("no large image", [](Req& r) { r.have.large = false; }, COREG_ESTATE, "pixels: the large and the small image must be set");
    refused("no small image", [](Req& r) { r.have.small = false; }, COREG_ESTATE, "pixels: the large and the small image must be set");
    refused("null plan", [](Req& r) { r.null_plan = true; }, COREG_EINVAL, "pixels: null pointer");
    refused("null output", [](Req& r) { r.null_out = true; }, COREG_EINVAL, "pixels: null pointer");
    refused("null dx list", [](Req& r) { r.null_dx = true; }, COREG_EINVAL, "pixels: null pointer");
    refused("no dy lag", [](Req& r) { r.dy.clear(); }, COREG_EINVAL, "pixels: empty lag axis");
    refused("ratio 0", [](Req& r) { r.pl.ratio1 = 0.0; }, COREG_EINVAL, "pixels: ratios and sub-resolved shape must be positive");
    refused("ratio NaN", [](Req& r) { r.pl.ratio2 = std::numeric_limits<double>::quiet_NaN(); }, COREG_EINVAL,
            "pixels: ratios and sub-resolved shape must be positive");
    refused("sub_nx 0", [](Req& r) { r.pl.sub_nx = 0; }, COREG_EINVAL, "pixels: ratios and sub-resolved shape must be positive");
    refused("tile of 13 rows", [](Req& r) { r.tiled = true; r.tile[0] = 13; }, COREG_EINVAL,
            "pixels: the tile shape must lie within [1, h] x [1, w] of the small image");
    refused("tile of 0 columns", [](Req& r) { r.tiled = true; r.tile[1] = 0; }, COREG_EINVAL,
            "pixels: the tile shape must lie within [1, h] x [1, w] of the small image");
    accepted("tile of the whole image", [](Req& r) { r.tiled = true; r.tile[0] = 12; r.tile[1] = 20; });
    refused("rotation lag inf", [](Req& r) { r.rot = {0.0, std::numeric_limits<double>::infinity()}; }, COREG_EINVAL,
            "pixels: a rotation lag is not finite");
    refused("box of 60008 x 60020", [](Req& r) { r.dx = {0, 60000}; r.dy = {0, 60000}; r.pl.sub_nx = r.pl.sub_ny = 100000; r.pl.l0 = r.pl.l1 = 0; },
            COREG_EINVAL, "pixels: work space too large");
    refused("2 tiles x 4096 x 65535 lags", [](Req& r) { r.dx.assign(4096, 0); r.dy.assign(65535, 0); r.tiled = true; r.tile[0] = 6; r.tile[1] = 20; },
            COREG_EINVAL, "pixels: too many tiles x lags");
    accepted("1 tile x 4096 x 65535 lags", [](Req& r) { r.dx.assign(4096, 0); r.dy.assign(65535, 0); r.tiled = true; r.tile[0] = 12; r.tile[1] = 20; });

    // either side of a limit
    accepted("l0 + min dy = 0", [](Req& r) { r.dy = {-10, 0}; });
    refused("l0 + min dy = -1", [](Req& r) { r.dy = {-11, 0}; }, COREG_EINVAL, kShift);
    accepted("l0 + max dy + h = sub_ny", [](Req& r) { r.dy = {0, 58}; });
    refused("l0 + max dy + h = sub_ny + 1", [](Req& r) { r.dy = {0, 59}; }, COREG_EINVAL, kShift);
    accepted("l1 + min dx = 0", [](Req& r) { r.dx = {0, -10}; });
    refused("l1 + min dx = -1", [](Req& r) { r.dx = {0, -11}; }, COREG_EINVAL, kShift);
    accepted("l1 + max dx + w = sub_nx", [](Req& r) { r.dx = {70, 0}; });
    refused("l1 + max dx + w = sub_nx + 1", [](Req& r) { r.dx = {71, 0}; }, COREG_EINVAL, kShift);
    accepted("65535 dy lags", [](Req& r) { r.dx = {0}; r.dy.assign(65535, 0); });
    refused("65536 dy lags", [](Req& r) { r.dx = {0}; r.dy.assign(65536, 0); }, COREG_EINVAL, "pixels: more than 65535 dy or rotation lags");
    refused("65536 rotation lags", [](Req& r) { r.dx = {0}; r.dy = {0}; r.rot.assign(65536, 0.0); }, COREG_EINVAL,
            "pixels: more than 65535 dy or rotation lags");
    // 255 tiles x 257 planes = 65535; 256 tiles x 256 planes = 65536
    accepted("65535 planes x tiles", [](Req& r) { r.have.w = 17; r.have.h = 15; r.tiled = true; r.tile[0] = r.tile[1] = 1; r.dx = {0}; r.dy = {0}; r.rot.assign(257, 0.0); });
    refused("65536 planes x tiles", [](Req& r) { r.have.w = 16; r.have.h = 16; r.tiled = true; r.tile[0] = r.tile[1] = 1; r.dx = {0}; r.dy = {0}; r.rot.assign(256, 0.0); },
            COREG_EINVAL, "pixels: more than 65535 rotation planes x tiles");
    accepted("65535 x 4096 lags", [](Req& r) { r.dx = {0}; r.dy.assign(65535, 0); r.rot.assign(4096, 0.0); });
    refused("65535 x 4097 lags", [](Req& r) { r.dx = {0}; r.dy.assign(65535, 0); r.rot.assign(4097, 0.0); }, COREG_EINVAL, "pixels: too many lags");
    accepted("step = tile", [](Req& r) { r.tiled = r.stepped = true; });
    accepted("step 1", [](Req& r) { r.tiled = r.stepped = true; r.step[0] = r.step[1] = 1; });
    refused("step = tile rows + 1", [](Req& r) { r.tiled = r.stepped = true; r.step[0] = 5; }, COREG_EINVAL, kStep);
    refused("step = tile columns + 1", [](Req& r) { r.tiled = r.stepped = true; r.step[1] = 6; }, COREG_EINVAL, kStep);
    refused("step 0", [](Req& r) { r.tiled = r.stepped = true; r.step[1] = 0; }, COREG_EINVAL, kStep);
    accepted("one positive weight per table", [](Req& r) { r.apodize(4, 5); r.wy = {0, 0, 1e-300, 0}; r.wx = {0, 0, 0, 0, 2}; });
    refused("weights all zero", [](Req& r) { r.apodize(4, 5); r.wx.assign(5, 0.0); }, COREG_EINVAL, "pixels: a weight table without a positive entry");
    refused("a negative weight", [](Req& r) { r.apodize(4, 5); r.wy[3] = -1e-300; }, COREG_EINVAL, kWeight);
    refused("a NaN weight", [](Req& r) { r.apodize(4, 5); r.wx[0] = std::numeric_limits<double>::quiet_NaN(); }, COREG_EINVAL, kWeight);
    refused("an infinite weight", [](Req& r) { r.apodize(4, 5); r.wy[0] = std::numeric_limits<double>::infinity(); }, COREG_EINVAL, kWeight);

    // two checks broken at once: the order of the checks
    refused("residus and a null plan", [](Req& r) { r.method = COREG_METHOD_RESIDUS; r.null_plan = true; }, COREG_ENOTIMPL,
            "pixels: method residus is not implemented (the reference's pxlshift has no such score); residus_masked is");
    refused("no bins and no images", [](Req& r) { r.method = COREG_METHOD_MUTUAL_INFORMATION; r.have = PixHave{false, false, 0, 0, 0, 0}; },
            COREG_ESTATE, kBins);
    refused("weighted residus_masked and a tile of 0 rows", [](Req& r) { r.apodize(0, 5); r.method = COREG_METHOD_RESIDUS_MASKED; },
            COREG_EINVAL, kCorrOnly);
}

// the grid and the counts of one stepped, tiled plan, by hand: 12 x 20 pixels, windows of 5 x 8 every 3 x 4
void one_plan() {
    Req r;
    r.tiled = r.stepped = true;
    r.tile[0] = 5;
    r.tile[1] = 8;
    r.step[0] = 3;
    r.step[1] = 4;
    r.rot = {0.0, 0.01};
    const PixPlan p = r.plan();
    CHECK(p.code == COREG_OK, "stepped plan refused");
    // rows: windows at 0, 3, 6, 9 (9 + 5 >= 12) -> 4; columns: 0, 4, 8, 12 (12 + 8 >= 20) -> 4
    CHECK(p.tl.n_tx == 4 && p.n_tiles == 16 && p.tl.n_tiles == 16 && p.tl.n_rot == 2, "stepped plan: %d x ... = %lld windows", p.tl.n_tx, p.n_tiles);
    CHECK(p.n_lag == 12 && p.n_out == 192, "stepped plan: %lld lags, %lld entries", p.n_lag, p.n_out);
    CHECK(p.grid[0] == 1 && p.grid[1] == 2 && p.grid[2] == 32 && p.fin_grid[0] == 1 && p.fin_grid[1] == 16, "stepped plan: grid");
    CHECK(p.min_dx == -1 && p.max_dx == 1 && p.min_dy == 0 && p.max_dy == 1 && p.bW == 22 && p.bH == 13, "stepped plan: box");
    CHECK(p.tiled && !p.lct && !p.mi && !p.resid && p.ts.sy == 3 && p.ts.sx == 4, "stepped plan: flags and step");
}
}  // namespace

int main() {
    groups();
    windows();
    bands();
    blobs();
    refusals();
    one_plan();
    if (n_bad) {
        std::printf("%d of %d checks failed\n", n_bad, n_checked);
        return 1;
    }
    std::printf("ok: pixels plan rules, %d checks\n", n_checked);
    return 0;
}
