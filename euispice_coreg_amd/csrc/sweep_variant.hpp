// Which k_sweep instantiation a sweep launch runs: the ONE list of the instantiated variants and the rule that picks one.
// Plain C++ with no HIP dependency (tests/native/sweep_variant_rules.cpp walks the rule on the host); included by
// libcoreg_hip.so's one translation unit before host_sweep_launch.hpp, which builds its table of kernels from the list.
#pragma once
#include <initializer_list>

namespace sweep_variant {

// (the values of MODE_* and ORDER_RT of kernels_common.hpp, asserted equal where both are visible)
constexpr int kTranslate = 0, kHomography = 1, kHomographySeries = 2, kCar = 3;
constexpr int kOrderRt = 0;  // the spline order is a launch uniform (orders 0, 4, 5 and whatever a mode does not compile)

struct SweepVariant {
    int mode, order;  // order: 1, 2, 3 or kOrderRt
    bool f32;         // pixel type of the image to align: float, else double
    bool round;       // samples rounded to float32 before the mask
    bool resid;       // method 'residus'
    int pitch;        // compile-time row pitch of the LDS window, 0: chosen per visit
};
constexpr bool operator==(const SweepVariant& a, const SweepVariant& b) {
    return a.mode == b.mode && a.order == b.order && a.f32 == b.f32 && a.round == b.round && a.resid == b.resid &&
           a.pitch == b.pitch;
}

constexpr int kNumSweepVariants = 71;
struct SweepVariantList {
    SweepVariant v[kNumSweepVariants] = {};
    int n = 0;
};
// 15 variants with a compile-time pitch (correlation only) + 16 + 12 + 12 + 16 generic ones: every (pixel type, method)
// of a compiled (mode, order), pitch per visit
constexpr SweepVariantList make_sweep_variants() {
    SweepVariantList l;
    auto pitched = [&l](int mode, int order, bool f32, std::initializer_list<int> pitches) {
        for (int p : pitches) l.v[l.n++] = SweepVariant{mode, order, f32, mode != kTranslate, false, p};
    };
    auto generic = [&l](int mode, std::initializer_list<int> orders) {
        for (int o : orders)
            for (int k = 0; k < 4; ++k) l.v[l.n++] = SweepVariant{mode, o, k < 2, mode != kTranslate, (k & 1) != 0, 0};
    };
    pitched(kTranslate, 2, true, {89, 121, 153, 185, 217});  // the common Carrington sweep
    pitched(kTranslate, 2, false, {89, 121, 153});           // the same with float64 pixels
    pitched(kTranslate, 3, true, {89, 121, 153});            // the cubic Carrington sweep
    pitched(kHomographySeries, 2, true, {89, 121});          // the common helioprojective sweeps
    pitched(kHomography, 2, true, {89, 121});
    generic(kTranslate, {1, 2, 3, kOrderRt});
    generic(kCar, {1, 2, kOrderRt});         // (no cubic plate-carree kernel: order 3 runs kOrderRt)
    generic(kHomographySeries, {1, 2, 3});   // (no kOrderRt: those orders run as kHomography)
    generic(kHomography, {1, 2, 3, kOrderRt});
    return l;
}
constexpr SweepVariantList kSweepVariants = make_sweep_variants();
static_assert(kSweepVariants.n == kNumSweepVariants, "the list of k_sweep variants has 71 entries");

// index of `v` in kSweepVariants, or -1
constexpr int sweep_variant_index(const SweepVariant& v) {
    for (int i = 0; i < kSweepVariants.n; ++i)
        if (kSweepVariants.v[i] == v) return i;
    return -1;
}

// The variant of a launch: mode and spline order of the sweep, pixel type of the image to align, method, and the pitch
// the host asks for (pick_pitch; 0: per visit).  The generic variant of (mode, order) compiles the order where the mode
// has it and reads it at run time otherwise -- a series homography of a run-time order is swept as kHomography; the
// requested pitch is honoured where the list holds that variant with it (correlation only), and dropped otherwise.
constexpr SweepVariant pick_sweep_variant(int mode, int order, bool small_f32, bool residus, int pitch_sel) {
    if (mode != kTranslate && mode != kCar && mode != kHomographySeries) mode = kHomography;
    const bool compiled = order == 1 || order == 2 || (order == 3 && mode != kCar);
    if (mode == kHomographySeries && !compiled) mode = kHomography;
    SweepVariant v{mode, compiled ? order : kOrderRt, small_f32, mode != kTranslate, residus, 0};
    if (pitch_sel > 0 && !residus) {
        v.pitch = pitch_sel;
        if (sweep_variant_index(v) < 0) v.pitch = 0;
    }
    return v;
}

}  // namespace sweep_variant
