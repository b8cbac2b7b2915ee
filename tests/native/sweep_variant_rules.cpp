// The rule that picks a k_sweep instantiation (csrc/sweep_variant.hpp) against an expectation written out here on its
// own, over 4 modes x orders 0..5 x {float32, float64} x {correlation, residus} x 7 requested pitches = 672 inputs:
// every result is the expected one, every result is an entry of the instantiation list, every entry of the list is
// reached, and the list has 71 distinct entries.  Host compiler only; prints "ok: ..." and returns 0, or says what differs.
#include <cstdio>

#include "../../euispice_coreg_amd/csrc/sweep_variant.hpp"

using namespace sweep_variant;

namespace {
// kernels_common.hpp: MODE_TRANSLATE = 0, MODE_HOMOGRAPHY = 1, MODE_HOMOGRAPHY_SERIES = 2, MODE_CAR = 3, ORDER_RT = 0
enum { TRANSLATE = 0, HOMOGRAPHY = 1, HOMOGRAPHY_SERIES = 2, CAR = 3, RT = 0 };

bool among(int x, std::initializer_list<int> set) {
    for (int s : set)
        if (s == x) return true;
    return false;
}

// the rules, restated: which pitches are compiled for which sweep, and which orders for which mode
SweepVariant expected(int mode, int order, bool f32, bool residus, int pitch_sel) {
    SweepVariant e;
    e.f32 = f32;
    e.resid = residus;
    e.round = mode != TRANSLATE;
    e.mode = mode;
    e.pitch = 0;
    if (!residus) {
        if (mode == TRANSLATE && order == 2 && f32 && among(pitch_sel, {89, 121, 153, 185, 217})) e.pitch = pitch_sel;
        if (mode == TRANSLATE && order == 2 && !f32 && among(pitch_sel, {89, 121, 153})) e.pitch = pitch_sel;
        if ((mode == HOMOGRAPHY || mode == HOMOGRAPHY_SERIES) && order == 2 && f32 && among(pitch_sel, {89, 121}))
            e.pitch = pitch_sel;
        if (mode == TRANSLATE && order == 3 && f32 && among(pitch_sel, {89, 121, 153})) e.pitch = pitch_sel;
    }
    switch (mode) {
        case TRANSLATE: e.order = among(order, {1, 2, 3}) ? order : RT; break;
        case CAR: e.order = among(order, {1, 2}) ? order : RT; break;
        case HOMOGRAPHY_SERIES:
            if (among(order, {1, 2, 3})) {
                e.order = order;
            } else {
                e.mode = HOMOGRAPHY;
                e.order = RT;
            }
            break;
        default: e.order = among(order, {1, 2, 3}) ? order : RT; break;
    }
    return e;
}

int n_bad = 0;
void check(bool ok, const char* what, int mode, int order, bool f32, bool residus, int pitch_sel, const SweepVariant& g) {
    if (ok) return;
    ++n_bad;
    std::printf("FAIL %s: mode %d order %d f32 %d residus %d pitch %d -> (%d, %d, %d, %d, %d, %d)\n", what, mode, order,
                (int)f32, (int)residus, pitch_sel, g.mode, g.order, (int)g.f32, (int)g.round, (int)g.resid, g.pitch);
}
}  // namespace

int main() {
    static_assert(kTranslate == TRANSLATE && kHomography == HOMOGRAPHY && kHomographySeries == HOMOGRAPHY_SERIES &&
                      kCar == CAR && kOrderRt == RT, "mode / order constants");
    int reached[kNumSweepVariants] = {0};
    int n = 0;
    for (int mode : {TRANSLATE, HOMOGRAPHY, HOMOGRAPHY_SERIES, CAR})
        for (int order = 0; order <= 5; ++order)
            for (int f32 = 0; f32 < 2; ++f32)
                for (int residus = 0; residus < 2; ++residus)
                    for (int pitch_sel : {0, 57, 89, 121, 153, 185, 217}) {
                        const SweepVariant g = pick_sweep_variant(mode, order, f32 != 0, residus != 0, pitch_sel);
                        const SweepVariant e = expected(mode, order, f32 != 0, residus != 0, pitch_sel);
                        ++n;
                        check(g == e, "differs from the rules", mode, order, f32, residus, pitch_sel, g);
                        // the asymmetries, spelled out
                        if (mode == CAR && order == 3)
                            check(g.mode == CAR && g.order == RT, "CAR order 3 is not ORDER_RT", mode, order, f32, residus, pitch_sel, g);
                        if (mode == HOMOGRAPHY_SERIES && among(order, {0, 4, 5}))
                            check(g.mode == HOMOGRAPHY && g.order == RT, "SERIES at a run-time order is not HOMOGRAPHY", mode,
                                  order, f32, residus, pitch_sel, g);
                        if (!f32 && among(pitch_sel, {185, 217}))
                            check(g.pitch == 0, "float64 at pitch 185 / 217 is pitched", mode, order, f32, residus, pitch_sel, g);
                        if (residus || pitch_sel == 57 || pitch_sel == 0)
                            check(g.pitch == 0, "pitched without a compiled pitch", mode, order, f32, residus, pitch_sel, g);
                        const int at = sweep_variant_index(g);
                        check(at >= 0 && at < kNumSweepVariants, "not in the instantiation list", mode, order, f32, residus,
                              pitch_sel, g);
                        if (at >= 0 && at < kNumSweepVariants) ++reached[at];
                    }
    if (n != 672) {
        ++n_bad;
        std::printf("FAIL: %d inputs walked, not 672\n", n);
    }
    if (kSweepVariants.n != 71) {
        ++n_bad;
        std::printf("FAIL: the list has %d entries, not 71\n", kSweepVariants.n);
    }
    int n_pitched = 0;
    for (int i = 0; i < kSweepVariants.n; ++i) {
        const SweepVariant& v = kSweepVariants.v[i];
        n_pitched += v.pitch > 0;
        if (!reached[i]) {
            ++n_bad;
            std::printf("FAIL: entry %d (%d, %d, %d, %d, %d, %d) is reached by no input\n", i, v.mode, v.order, (int)v.f32,
                        (int)v.round, (int)v.resid, v.pitch);
        }
        if (sweep_variant_index(v) != i) {  // (the first match: an entry listed twice would find its earlier copy)
            ++n_bad;
            std::printf("FAIL: entry %d is listed twice\n", i);
        }
    }
    if (n_pitched != 15) {
        ++n_bad;
        std::printf("FAIL: %d pitched entries, not 15\n", n_pitched);
    }
    if (n_bad) return 1;
    std::printf("ok: %d inputs, %d variants (%d pitched), all reached\n", n, kSweepVariants.n, n_pitched);
    return 0;
}
