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

// RacingTrajectory::global_to_frenet for one pose (px, py, phi), the body of lmpc_track_project_kernel (lmpc_track_kernel.hip has the
// method's description) and of the projection step of lmpc_estimated_loop_kernel: the seed `s` where have_seed, else the abscissa
// of the nearest waypoint; Newton on g(s) = (r(s) - p) . r'(s); the outputs as the host class forms them.  The waypoint loop is
// wave-uniform over the lanes that CALL this (every lane of a wave that has one unseeded lane walks it): call it from code that
// every lane whose result is wanted reaches together.  No lane reads another's data.
struct track_frenet {
  double s, t, xi;
  int status;
};
__device__ __forceinline__ track_frenet track_project(const lmpc_spline_view& T, double px, double py, double phi, double s, bool have_seed) {
#pragma clang fp contract(off)
  const bool bad = !(isfinite(px) && isfinite(py) && isfinite(phi));
  if (bad) px = T.wp_xy[0], py = T.wp_xy[1], phi = 0.0;
  if (__any(!have_seed)) {
    double best = INFINITY;
    int ibest = 0;
#pragma unroll 4
    for (int j = 0; j < T.n_wp; ++j) {
      const double wx = T.wp_xy[2 * (size_t)j], wy = T.wp_xy[2 * (size_t)j + 1];  // wave-uniform address: scalar loads
      const double d = (wx - px) * (wx - px) + (wy - py) * (wy - py);
      if (d < best) best = d, ibest = j;
    }
    if (!have_seed) s = T.wp_s[ibest];
  }
  const double hbar = T.hbar, tol = 1e-13 * fmax(1.0, T.L);
  int piece = 0, st = LMPC_TRACK_NOT_CONVERGED;
  s = track_mod(s, T.L);
  track_point r = track_eval(T, s, piece);
  double ex = r.x - px, ey = r.y - py;
  double g = ex * r.dx + ey * r.dy;
  for (int it = 0; it < 30; ++it) {
    const double v2 = r.dx * r.dx + r.dy * r.dy;
    const double H = v2 + (ex * r.d2x + ey * r.d2y);
    double step = H > 1e-3 * v2 ? -g / H : -(double)((g > 0.0) - (g < 0.0)) * hbar;
    step = fmin(fmax(step, -2.0 * hbar), 2.0 * hbar);
    double a = 1.0, sn, gn;
    track_point rn;
    for (int k = 0;; ++k) {
      sn = s + a * step;
      rn = track_eval(T, sn, piece);
      gn = (rn.x - px) * rn.dx + (rn.y - py) * rn.dy;
      if (!(fabs(gn) > fabs(g)) || k == 6) break;
      a *= 0.5;
    }
    s = sn, r = rn, g = gn;
    ex = r.x - px, ey = r.y - py;
    if (fabs(a * step) < tol) {
      st = 0;
      break;
    }
  }
  // the outputs, exactly as the host class forms them (racing_trajectory.cpp:170-180)
  const double so = track_mod(s, T.L);
  const track_point o = track_eval(T, so, piece);
  const double yaw = atan2(o.dy, o.dx);
  const double sg = cos(yaw) * (py - o.y) - sin(yaw) * (px - o.x);  // lateral_sign (utils.hpp)
  double t = hypot(px - o.x, py - o.y) * (double)((sg > 0.0) - (sg < 0.0));
  double xi = track_align_yaw(phi, yaw) - yaw;
  double s_out = so;
  if (bad) s_out = t = xi = NAN, st = LMPC_TRACK_BAD_INPUT;
  return {s_out, t, xi, st};
}

// RacingTrajectory::frenet_to_global for one (s, e_y, e_psi): the body of lmpc_track_to_global_kernel
struct track_pose {
  double x, y, yaw;
};
__device__ __forceinline__ track_pose track_to_global(const lmpc_spline_view& T, double s, double t, double xi) {
#pragma clang fp contract(off)
  int piece = 0;
  const track_point r = track_eval(T, s, piece);
  const double yaw0 = atan2(r.dy, r.dx);
  return {r.x - sin(yaw0) * t, r.y + cos(yaw0) * t, track_align_yaw(yaw0 + xi, 0.0)};
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
