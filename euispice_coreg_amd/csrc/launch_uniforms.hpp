// What the kernels and the host's sweep planner (sweep_plan.hpp) both need to know of a launch: the tile and batch sizes,
// the coordinate-map modes and the per-launch uniforms.  Plain C++ with no HIP dependency: kernels_common.hpp includes it
// for the device side, sweep_plan.hpp for the host's.
#pragma once
namespace coreg {

#ifndef COREG_TILE_PTS
#define COREG_TILE_PTS 1024
#endif
constexpr int kTilePts = COREG_TILE_PTS;  // grid points per tile
constexpr int kBlock = 256;     // lag slots per batch (one lag per lane, 4 waves)

// MODE_HOMOGRAPHY_SERIES: same map, denominator 1 + eps inverted as 1 - eps + eps^2 (host guarantees |eps| < 4e-6, i.e.
// a truncation error below 1e-16 relative); MODE_HOMOGRAPHY divides exactly (any field of view)
// MODE_CAR: plate-carree maps on both sides (align_using_initial_carrington): base coordinates = native (phi, theta) of
// the target pixel [radians], per lag a rotation of the sphere (h[0..8]) between the two native frames, then
// (atan2, asin) and the affine native -> pixel map of the shifted header (uniform per launch, LaunchU)
enum { MODE_TRANSLATE = 0, MODE_HOMOGRAPHY = 1, MODE_HOMOGRAPHY_SERIES = 2, MODE_CAR = 3 };
// per-launch uniforms of the coordinate map / sampler that are not per-lane
struct LaunchU {
    double m00, m01, m10, m11, b0, b1;  // MODE_CAR: native (phi, theta) [rad] -> 0-based pixel
    int order_rt;                       // ORDER == ORDER_RT kernels: the spline order (0..5)
    int h_incr;                         // HOMOGRAPHY[_SERIES], order 2, interior LDS visits: advance along runs (tile_points)
    double box_c;     // MODE_CAR: (tile half-diagonal [rad])^2 / 2 x pixels per radian of the shifted map (car_tile_margin)
    double pole_sep;  // MODE_CAR: largest angle [rad] between the native poles of the target and of a shifted map
};

}  // namespace coreg
