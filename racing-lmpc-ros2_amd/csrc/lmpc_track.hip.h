// lmpc_track.hip.h -- the track on the device, as every kernel file evaluates it: the piecewise cubics of an lmpc_spline_track
// (RacingTrajectory's interpolants: wrapped abscissa, piece lookup, Horner forms, the centre line and its derivatives, align_yaw)
// and the periodic linear lookup into the uniform tables of an lmpc_track.  Included by lmpc_track_kernel.hip (the three track
// kernels), lmpc_prep_kernels.hip (the plant, the shift, the preparation) and lmpc_vanilla_kernel.hip (pure pursuit + plant).
// Contraction is off in everything that evaluates a spline, so that every kernel computes r(s) with the same roundings (and the
// same as the host classes): a pose made by one kernel projects back onto its abscissa through another.
#ifndef LMPC_TRACK_HIP_H_
#define LMPC_TRACK_HIP_H_

#include <hip/hip_runtime.h>

#include <math.h>

#include "lmpc_device.h"

#define LMPC_TRACK_COEF 20  // doubles per piece

// what the kernels take of an lmpc_spline_track (csrc/lmpc_capi.hip owns the buffers)
struct lmpc_spline_view {
  double L;      // total length
  double hbar;   // median waypoint spacing
  int P;         // pieces; breaks [P + 1]
  int n_wp;      // waypoints
  const double* breaks;
  const double* coef;   // [P][LMPC_TRACK_COEF]
  const double* wp_xy;  // [n_wp][2]
  const double* wp_s;   // [n_wp]
};

// align_abscissa(s, L/2, L): lmpc_utils/utils.hpp:35-41 -- the abscissa every interpolant is evaluated at (racing_trajectory.cpp:98)
__device__ __forceinline__ double track_mod(double s, double L) {
#pragma clang fp contract(off)
  const double s2 = L / 2.0;
  const double k = fabs(s2 - s) + L / 2.0;
  const double l = k - fmod(k, L);
  return s + l * (double)((s2 > s) - (s2 < s));
}

// The last piece whose left break is <= sm (the end pieces extrapolate): binary search over breaks [0 .. P], started from `hint`
// (a piece index in [0, P)).  Terminates whatever sm is: the interval shrinks on either outcome of the comparison.
__device__ __forceinline__ int track_piece(const double* __restrict__ breaks, int P, double sm, int hint) {
  const double left = breaks[hint];
  if (left <= sm && (hint == P - 1 || sm < breaks[hint + 1])) return hint;
  int lo = left <= sm ? hint : 0, hi = left <= sm ? P : hint;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (breaks[mid] <= sm) lo = mid; else hi = mid;
  }
  return lo;
}

struct track_poly {
  double a, b, c, d;
};
__device__ __forceinline__ track_poly track_load(const double* __restrict__ coef, int piece, int which) {
  const double2* p = reinterpret_cast<const double2*>(coef + (size_t)piece * LMPC_TRACK_COEF + 4 * which);  // 32-byte aligned
  const double2 lo = p[0], hi = p[1];
  return {lo.x, lo.y, hi.x, hi.y};
}
// NotAKnotCubic::operator() (host/racing_trajectory.cpp): value, first and second derivative, in the host's Horner forms
__device__ __forceinline__ double poly0(const track_poly& q, double h) {
#pragma clang fp contract(off)
  return q.a + h * (q.b + h * (q.c + h * q.d));
}
__device__ __forceinline__ double poly1(const track_poly& q, double h) {
#pragma clang fp contract(off)
  return q.b + h * (2.0 * q.c + 3.0 * h * q.d);
}
__device__ __forceinline__ double poly2(const track_poly& q, double h) {
#pragma clang fp contract(off)
  return 2.0 * q.c + 6.0 * h * q.d;
}

// the centre line and its derivatives at abscissa s (wrapped here); `piece` in: where to start the lookup, out: the piece used
struct track_point {
  double x, y, dx, dy, d2x, d2y;
};
__device__ __forceinline__ track_point track_eval(const lmpc_spline_view& T, double s, int& piece) {
#pragma clang fp contract(off)
  const double sm = track_mod(s, T.L);
  piece = track_piece(T.breaks, T.P, sm, piece);
  const double h = sm - T.breaks[piece];
  const track_poly qx = track_load(T.coef, piece, 0), qy = track_load(T.coef, piece, 1);
  return {poly0(qx, h), poly0(qy, h), poly1(qx, h), poly1(qy, h), poly2(qx, h), poly2(qy, h)};
}

// utils.hpp:25-31
__device__ __forceinline__ double track_align_yaw(double yaw_1, double yaw_2) {
#pragma clang fp contract(off)
  const double d = yaw_1 - yaw_2;
  return atan2(sin(d), cos(d)) + yaw_2;
}

// periodic linear interpolation on a uniform table of M samples over [0, L)
__device__ __forceinline__ double track_lookup(const double* __restrict__ tab, int M, double L, double s) {
  double u = fmod(s, L);
  if (u < 0.0) u += L;
  u = u / (L / M);
  double fl = floor(u);
  const double fr = u - fl;
  int i0 = (int)fl;
  i0 = i0 % M;
  if (i0 < 0) i0 += M;
  const int i1 = (i0 + 1 == M) ? 0 : i0 + 1;
  return tab[i0] * (1.0 - fr) + tab[i1] * fr;
}

#endif  // LMPC_TRACK_HIP_H_
