// lmpc_estimated_loop_kernel.hip -- everything between two solves of the ESTIMATED closed loop in one launch
// (lmpc_loop_advance_estimated_batch, include/lmpc_hip_estimated.h): closed_loop.run_estimated's loop body from the solve of period k
// to just before the solve of period k + 1.  Per car, in order:
//   1 the input applied (to u_prev and to the filter's control), 2 the truth's first half period, 3 the velocity observation and the
//   filter's update by it, 4 the truth's second half period and the books, 5 the pose observation and the update by it, 6 the squared
//   error of the estimate, 7 the estimate's projection to the Frenet frame (the next x_ic), 8 the next references -- the shifted
//   solution, or for a failed car the old plan shifted in place or the cold restart at the new x_ic.
// Every step is the text the stand-alone kernel is made of: 2, 4 and the failed car's routes of 8 the macros of
// lmpc_loop_steps.hip.h, 3 and 5 the functions of lmpc_ekf_steps.hip.h, 5 and 7 those of lmpc_track.hip.h, the shifted solution
// lmpc_car_shift_knot.
//
// Shape: one thread per car, the batch on the lanes, a workgroup of one wave; every access to a [field][knot][B] array is a
// coalesced wave transaction.  No LDS, no barrier, and no cross-lane traffic but the wave-uniform waypoint search of the projection
// (walked only by a wave with a car whose incoming x_ic[0] is not finite).  The cars past the batch leave at the first statement.
// The truth lives in registers across the two halves; the filter's state stays in its store in global memory, where each step reads
// back what the same thread wrote.  Ordinary vector loads and stores.
//
// One kernel, not two: the resource report (profiles/estimated_fused.md) shows the chain at the prediction's registers -- the live
// set outside the prediction is the truth, the input and a handful of scalars -- and the scratch is that of the out-of-line
// rollouts, as in lmpc_fleet_loop_kernel.
#include <hip/hip_runtime.h>

#include "lmpc_ekf_steps.hip.h"
#include "lmpc_estimated.h"
#include "lmpc_loop_steps.hip.h"

namespace {

// The three rollouts, OUT OF LINE and in the form lmpc_fleet_loop_kernel.hip gives them (its comment has the measurements): vehicle,
// table and arrays by value, the scratch arrays their own, around the one text of lmpc_loop_steps.hip.h.  A call's code does not
// depend on its caller, so the contraction inside the model is the same whatever this kernel does around it, and the results are held
// bit for bit to lmpc_plant_kernel, lmpc_prepare_kernel and lmpc_shift_kernel (tests/test_gpu_estimated_loop.py).
__device__ __noinline__ void est_loop_plant(lmpc_vehicle veh, lmpc_track trk, double* __restrict__ x_io, double u0, double u1, double dt_sim,
                                            int nsub) {
  double x[6], xn[6];
  const double u[2] = {u0, u1};
#pragma unroll
  for (int k = 0; k < 6; ++k) x[k] = x_io[k];
  LMPC_PLANT_SUBSTEPS(veh, trk, x, u, dt_sim, nsub, xn)
#pragma unroll
  for (int k = 0; k < 6; ++k) x_io[k] = x[k];
}
__device__ __noinline__ void est_loop_cold_restart(lmpc_vehicle veh, lmpc_track trk, lmpc_ref_arrays r, int b, int B, int N, double x0, double x1,
                                                   double x2, double x3, double x4, double x5, double dt, double d, double speed_scale,
                                                   double speed_limit) {
  double x[6] = {x0, x1, x2, x3, x4, x5}, xn[6];
  LMPC_CAR_COLD_RESTART(veh, trk, r, b, B, N, x, xn, dt, d, speed_scale, speed_limit)
}
__device__ __noinline__ void est_loop_shift_in_place(lmpc_vehicle veh, lmpc_track trk, lmpc_ref_arrays r, int b, int B, int N, double dt, double d,
                                                     double speed_scale, double speed_limit) {
  double x[6], xn[6], u[2] = {0.0, 0.0};
  LMPC_CAR_SHIFT_IN_PLACE(veh, trk, r, b, B, N, x, xn, u, dt, d, speed_scale, speed_limit)
}

// One update of car b's filter by the measurement zv (the prediction over dt, then the correction): lmpc_ekf_launch's two kernels,
// the branch on the observation's row count uniform over the launch.  xe [6] out: the new estimate.  Returns the car's flags.
__device__ __forceinline__ int est_loop_update(const lmpc_estimated_consts& K, const lmpc_ekf_store& st, const lmpc_ekf_obs& ob, int b, double dt,
                                               const double* zv, const double* __restrict__ R, double* xe) {
  const lmpc_ekf_out none{nullptr, nullptr, nullptr, nullptr};
  lmpc_ekf_predict_car(K.veh, K.ekf, st, b, dt, 0, none);
  switch (ob.nz) {
    case 1: return lmpc_ekf_correct_car<1>(K.ekf, st, ob, b, zv, R, none, xe);
    case 2: return lmpc_ekf_correct_car<2>(K.ekf, st, ob, b, zv, R, none, xe);
    default: return lmpc_ekf_correct_car<3>(K.ekf, st, ob, b, zv, R, none, xe);
  }
}

// one of three values by a row index the launch shares (selects: nothing in registers is indexed at run time)
__device__ __forceinline__ double est_pick(int row, double a0, double a1, double a2) { return row == 0 ? a0 : (row == 1 ? a1 : a2); }

__global__ __launch_bounds__(64) void lmpc_estimated_loop_kernel(lmpc_estimated_consts K, lmpc_ekf_store st, lmpc_track trk, lmpc_spline_view T,
                                                                 lmpc_estimated_loop io) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  const int Bi = st.B, N = K.N, NS = N - 1;
  if (b >= Bi) return;
  const size_t B = (size_t)Bi;
  const bool ok = io.status[b] == 0;
  const lmpc_ref_arrays refs{io.X_ref, io.U_ref, io.T_ref, io.bound_left, io.bound_right, io.curvatures, io.vel_ref};
  const double d = K.max_vel_ref_diff;
  const int half = io.n_sub / 2;
  // ---- 1 the input applied: to the plant, to the next solve and to the filter (update_control) ----
  double x[6], u[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    u[k] = ok ? io.U_optm[(size_t)(k * NS) * B + b] : io.U_ref[(size_t)(k * NS) * B + b];
    io.u_prev[(size_t)k * B + b] = u[k];
    st.u[(size_t)k * B + b] = u[k];
  }
  if (io.n_fail && !ok) io.n_fail[b] += 1;
  // ---- 2 the truth, first half ----
#pragma unroll
  for (int k = 0; k < 6; ++k) x[k] = io.x[(size_t)k * B + b];
  const double s_before = x[0];
  est_loop_plant(K.veh, trk, x, u[0], u[1], io.dt_sim, half);
  // ---- 3 the velocity observation (rows within 3 .. 5) and the update by it ----
  double zv[3], xe[6];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    zv[a] = 0.0;
    if (a < K.obs_vel.nz) {
      zv[a] = est_pick(K.obs_vel.rows[a] - 3, x[3], x[4], x[5]) + io.noise_vel[(size_t)a * B + b];
      if (io.z_vel) io.z_vel[(size_t)a * B + b] = zv[a];
    }
  }
  int flags = est_loop_update(K, st, K.obs_vel, b, K.dt_vel, zv, io.R_vel, xe);
  // ---- 4 the truth, second half; the books (lmpc_loop_advance_kernel's) ----
  est_loop_plant(K.veh, trk, x, u[0], u[1], io.dt_sim, half);
#pragma unroll
  for (int k = 0; k < 6; ++k) io.x[(size_t)k * B + b] = x[k];
  if (io.distance) {
    const double ds = x[0] - s_before;
    io.distance[b] += (ds < -trk.L / 2.0) ? ds + trk.L : ds;
  }
  if (io.worst_excess) {
    const double half_b = K.veh.b / 2.0;
    const double exc = fmax(x[1] + half_b - io.bound_left[b], io.bound_right[b] - (x[1] - half_b));  // (knot 0 of the period just driven)
    io.worst_excess[b] = fmax(io.worst_excess[b], exc);
  }
  // ---- 5 the pose observation (rows within 0 .. 2; a yaw row in (-pi, pi]) and the update by it ----
  const track_pose pose = track_to_global(T, x[0], x[1], x[2]);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    zv[a] = 0.0;
    if (a < K.obs_pose.nz) {
      const int row = K.obs_pose.rows[a];
      zv[a] = est_pick(row, pose.x, pose.y, pose.yaw) + io.noise_pose[(size_t)a * B + b];
      if (row == 2) zv[a] = atan2(sin(zv[a]), cos(zv[a]));
      if (io.z_pose) io.z_pose[(size_t)a * B + b] = zv[a];
    }
  }
  flags |= est_loop_update(K, st, K.obs_pose, b, K.dt_pose, zv, io.R_pose, xe);
  if (io.ekf_flags) io.ekf_flags[b] |= flags;
  if (io.x_est) {
#pragma unroll
    for (int k = 0; k < 6; ++k) io.x_est[(size_t)k * B + b] = xe[k];
  }
  // ---- 6 the squared error of the estimate in the global frame, the yaw difference wrapped ----
  if (io.sq_err) {
#pragma clang fp contract(off)
    const double truth[6] = {pose.x, pose.y, pose.yaw, x[3], x[4], x[5]};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      double e = xe[k] - truth[k];
      if (k == 2) e = atan2(sin(e), cos(e));
      io.sq_err[(size_t)k * B + b] += e * e;
    }
  }
  // ---- 7 the controller's next state: the estimate's pose projected from the abscissa the last solve was given ----
  const double s0 = io.x_ic[b];
  const track_frenet f = track_project(T, xe[0], xe[1], xe[2], s0, isfinite(s0));
  const double xic[6] = {f.s, f.t, f.xi, xe[3], xe[4], xe[5]};
#pragma unroll
  for (int k = 0; k < 6; ++k) io.x_ic[(size_t)k * B + b] = xic[k];
  if (io.track_status) io.track_status[b] = max(io.track_status[b], f.status);
  // ---- 8 the next references (lmpc_loop_steps.hip.h) ----
  // The cars whose solve succeeded FIRST, the failed cars' out-of-line routes LAST, with nothing of the kernel behind them.  The
  // order is load-bearing.  est_loop_shift_in_place takes all 256 VGPRs, so around its call the compiler parks the registers that
  // hold this kernel's spilled SGPRs in AGPRs, written in every lane of the wave; with the succeeded cars' loop BEHIND the call it
  // chose the AGPR in which those (then inactive) lanes kept their car index, and their stores went to wild addresses -- an illegal
  // memory access on the first run with restart_failed = 0, read off the assembly (v_accvgpr_write_b32 a4, v255 under
  // s_or_saveexec -1, a4 read again by the loop).  Behind the failed cars' calls no lane has anything left to do.  The wave barrier
  // between the two is no instruction: it is a convergent operation, which keeps the compiler from folding the two conditions back
  // into one if / else and laying the loop out behind the calls again.
  if (ok) {
    double xk[6];
    for (int i = 0; i < N; ++i) lmpc_car_shift_knot(K.veh, trk, refs, b, Bi, N, i, io.X_optm, io.U_optm, xk, io.dt, d, io.speed_scale, io.speed_limit);
  }
  __builtin_amdgcn_wave_barrier();
  if (!ok) {
    if (io.restart_failed)  // cold start at the new ESTIMATE (lmpc_prepare_kernel)
      est_loop_cold_restart(K.veh, trk, refs, b, Bi, N, xic[0], xic[1], xic[2], xic[3], xic[4], xic[5], io.dt, d, io.speed_scale, io.speed_limit);
    else  // the plan the failed solve started from, shifted in place (lmpc_shift_kernel with X_old = X_ref)
      est_loop_shift_in_place(K.veh, trk, refs, b, Bi, N, io.dt, d, io.speed_scale, io.speed_limit);
  }
}

}  // namespace

hipError_t lmpc_estimated_launch(hipStream_t stream, const lmpc_estimated_consts& K, const lmpc_ekf_store& st, const lmpc_track& trk,
                                 const lmpc_spline_view& spline, const lmpc_estimated_loop& io) {
  hipLaunchKernelGGL(lmpc_estimated_loop_kernel, dim3((st.B + 63) / 64), dim3(64), 0, stream, K, st, trk, spline, io);
  return hipGetLastError();
}
