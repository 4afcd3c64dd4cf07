// lmpc_track_kernel.hip -- the track's interpolating splines on the device: global <-> Frenet for a batch of poses.
//
// RacingTrajectory (racing_trajectory.cpp:25-236) fits five not-a-knot cubics -- x, y, speed, left and right boundary offset -- through
// the waypoints over their abscissa and derives yaw = atan2(y', x') and the curvature expression as written (:108-110); every
// interpolant is evaluated at align_abscissa(s, L/2, L) (:98).  The banded solve stays on the host, once per track
// (RacingTrajectory::to_spline_track); what arrives here is the piecewise polynomials a + b h + c h^2 + d h^3 over the P + 1 breaks of
// the extended waypoint abscissae, repacked by lmpc_spline_track_create as one 160-byte record per piece
//     coef[piece] = x[4] | y[4] | vel[4] | left[4] | right[4]
// so that the projection gathers a piece's x and y coefficients as one 64-byte line.  Three kernels:
//   lmpc_track_project_kernel    global_to_frenet (:204-236; called by RacingMPCNode::on_step_timer, racing_mpc_node.cpp:181-185, and by
//                                the simulator node, racing_simulator_node.cpp:60-65), one lane per pose
//   lmpc_track_to_global_kernel  frenet_to_global (:122-186; frenet_to_global_function().map(N), racing_mpc_node.cpp:50,460), one
//                                thread per (knot, problem)
//   lmpc_track_sample_kernel     the seven interpolants at arbitrary abscissae, or at s_j = j L / M into the tables of an lmpc_track
// Contraction is off in everything that evaluates a spline: the three kernels then compute r(s) with the same roundings (and the
// same as the host classes), so that a pose made by one kernel projects back onto its abscissa through another.
//
// The tables are small (BARC: 159 pieces, 25 KB; 1400 waypoints: 225 KB) and read-only: they are gathered from global memory and
// stay in L2.  (Staging the breaks and the x / y coefficients in LDS was not built: 72 KB at 1400 waypoints would cap a CU at
// two workgroups for a kernel whose launch, not its loads, is what a batch of 4096 pays for -- DESIGN.md section 4.)
#include <hip/hip_runtime.h>

#include <math.h>

#include "lmpc_device.h"

#include "lmpc_track.hip.h"

// RacingTrajectory::global_to_frenet for B poses, pose [3][B] = (x, y, yaw) -> frenet [3][B] = (s, t, xi), status [B].
// Seed: s0[b] where s0 != NULL and (seeded == NULL or seeded[b] != 0) and s0[b] is finite; else the abscissa of the nearest
// waypoint, first index on ties (the kd-tree lookup upstream, :213-216).  The waypoint loop is wave-uniform: a waypoint arrives by
// scalar loads and every lane tests its own distance; a wave whose lanes are all seeded skips it.
// Iteration: Newton on the first-order condition g(s) = (r(s) - p) . r'(s) of the distance the reference minimises (:144-169, CasADi
// sqpmethod), H = |r'|^2 + (r - p) . r'': step -g / H where H > 1e-3 |r'|^2, else -sign(g) hbar; |step| <= 2 hbar; the step is halved
// while |g| grows, at most 6 times; stop when the step taken is below 1e-13 max(1, L); 30 iterations at most
// (LMPC_TRACK_NOT_CONVERGED).  Every evaluation wraps its abscissa, so the iterate never walks onto the +L copies of the first pieces.
// A non-finite pose is LMPC_TRACK_BAD_INPUT with NaN outputs: its lane iterates on the first waypoint instead, so that every loop
// below runs on finite values, and no lane reads another's data.
__global__ __launch_bounds__(64) void lmpc_track_project_kernel(lmpc_spline_view T, int B, const double* __restrict__ pose,
                                                                const double* __restrict__ s0, const int* __restrict__ seeded,
                                                                double* __restrict__ frenet, int* __restrict__ status) {
#pragma clang fp contract(off)
  const int gb = blockIdx.x * 64 + threadIdx.x;
  const bool live = gb < B;
  const int b = live ? gb : B - 1;
  const double px = pose[b], py = pose[(size_t)B + b], phi = pose[2 * (size_t)B + b];
  double s = 0.0;
  bool have_seed = false;
  if (s0 && (!seeded || seeded[b] != 0)) {
    s = s0[b];
    have_seed = isfinite(s);
  }
  const track_frenet f = track_project(T, px, py, phi, s, have_seed);  // (every lane: the cars past the batch redo the last one)
  if (live) {
    frenet[b] = f.s;
    frenet[(size_t)B + b] = f.t;
    frenet[2 * (size_t)B + b] = f.xi;
    status[b] = f.status;
  }
}

// RacingTrajectory::frenet_to_global for rows 0 - 2 (s, e_y, e_psi) of an SOA state array X [6][n][B] -> pose [3][n][B] = (x, y, yaw);
// one thread per (knot, problem), `count` = n B of them.
__global__ __launch_bounds__(256) void lmpc_track_to_global_kernel(lmpc_spline_view T, long long count, const double* __restrict__ X,
                                                                   double* __restrict__ pose) {
#pragma clang fp contract(off)
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  const double s = X[e], t = X[count + e], xi = X[2 * count + e];
  const track_pose p = track_to_global(T, s, t, xi);
  pose[e] = p.x;
  pose[count + e] = p.y;
  pose[2 * count + e] = p.yaw;
}

// The interpolants at abscissa s[j] (s != NULL) or at s_j = j L / n, the sample points of an lmpc_track with M = n (s == NULL).
// Any output may be NULL.  curvature: x' y'' - y' x'' / sqrt((x'^2 + y'^2)^3), as written (:108-110).
__global__ __launch_bounds__(256) void lmpc_track_sample_kernel(lmpc_spline_view T, int n, const double* __restrict__ s_in,
                                                                double* __restrict__ x, double* __restrict__ y, double* __restrict__ yaw,
                                                                double* __restrict__ curvature, double* __restrict__ left,
                                                                double* __restrict__ right, double* __restrict__ vel) {
#pragma clang fp contract(off)
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const double s = s_in ? s_in[j] : T.L * (double)j / (double)n;
  int piece = 0;
  const track_point r = track_eval(T, s, piece);
  const double h = track_mod(s, T.L) - T.breaks[piece];
  if (x) x[j] = r.x;
  if (y) y[j] = r.y;
  if (yaw) yaw[j] = atan2(r.dy, r.dx);
  if (curvature) {
    const double v2 = r.dx * r.dx + r.dy * r.dy;
    curvature[j] = r.dx * r.d2y - r.dy * r.d2x / sqrt(v2 * v2 * v2);
  }
  if (vel) vel[j] = poly0(track_load(T.coef, piece, 2), h);
  if (left) left[j] = poly0(track_load(T.coef, piece, 3), h);
  if (right) right[j] = poly0(track_load(T.coef, piece, 4), h);
}
