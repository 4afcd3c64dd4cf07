// lmpc_vanilla_kernel.hip -- the batched vanilla controller, one per car: pure pursuit for the steering, a PID on the speed for the
// longitudinal force (VanillaController::solve, vanilla_controller.cpp:49-109; PidController::update, pid_controller.cpp:83-127),
// and the kernel that runs controller and plant for many control periods in one launch.  See lmpc_vanilla.h and, for the formulas,
// lmpc_vanilla_create in include/lmpc_hip.h.
//
// Three kernels, all __launch_bounds__(64), ONE LANE PER CAR, fp64:
//   lmpc_vanilla_solve_kernel    one control decision per car; reads and writes the PID state
//   lmpc_vanilla_rollout_kernel  `periods` control periods per car: the decision, then n_sub plant sub-steps (the arithmetic of
//                                lmpc_plant_kernel), logs and accumulators; x and the PID state are updated in place
//   lmpc_vanilla_fleet_kernel    the rollout with a plant per car and the fleet safe set's recorder in the period loop
//                                (include/lmpc_hip_vanilla_fleet.h), a template over (plant kind, recording on / off)
// The work is a serial chain per car -- two spline evaluations, a handful of transcendental calls, and in the rollout 4 n_sub model
// evaluations per period, each waiting for the last -- and the only parallelism is across cars.  A workgroup is one wave so that
// 4096 cars are 64 workgroups on 64 CUs instead of 16 workgroups of four waves on 16; nothing is shared between lanes: no LDS, no
// cross-lane operation, no barrier.  The spline tables are gathered from global memory and stay in L2 (lmpc_track_kernel.hip).
//
// Every loop count is a constant, n_sub or periods (track_piece's search shrinks its interval on either outcome of a comparison),
// so a NaN or 1e300 input cannot lengthen a launch.  A car whose decision is not finite is flagged, its PID state is left as it was
// and, in the rollout, it is frozen: the plant is never stepped from a state the decision refused.  No lane reads another car's data.
//
// Contraction is off in the decision and in the logged table lookups: the decision then has the same bits in both kernels, and
// k_log, the bounds of worst_excess and every intermediate of the decision can be reproduced on the host operation by operation.
// The plant sub-step keeps the default, as lmpc_plant_kernel has it (see vanilla_plant).
#include <hip/hip_runtime.h>

#include <math.h>

#include "lmpc_cars.h"
#include "lmpc_device.h"
#include "lmpc_dtrack_dynamics.hip.h"
#include "lmpc_dynamics.hip.h"
#include "lmpc_loop_steps.hip.h"
#include "lmpc_track.hip.h"
#include "lmpc_vanilla.h"

namespace {

// std::clamp(v, lo, hi) as the standard library evaluates it: a NaN v passes through
__device__ __forceinline__ double vanilla_clamp(double v, double lo, double hi) { return (v < lo) ? lo : ((hi < v) ? hi : v); }

struct vanilla_pid {
  double integral, error, last_error;
};

struct vanilla_decision {
  double FD, FB, steer;  // u_out
  double um0;            // u_model[0] = u_a force_to_lon (u_model[1] = steer)
  vanilla_pid pid;       // the PID state after the call (valid where `finite`)
  bool finite;
};

// track_lookup's formula with contraction off: what the logs and the bounds of worst_excess use, so that the host reproduces them
__device__ __forceinline__ double vanilla_lookup(const double* __restrict__ tab, int M, double L, double s) {
#pragma clang fp contract(off)
  double u = fmod(s, L);
  if (u < 0.0) u += L;
  u = u / (L / M);
  const double fl = floor(u);
  const double fr = u - fl;
  int i0 = (int)fl;
  i0 = i0 % M;
  if (i0 < 0) i0 += M;
  const int i1 = (i0 + 1 == M) ? 0 : i0 + 1;
  return tab[i0] * (1.0 - fr) + tab[i1] * fr;
}

// One control decision.  x: the car's state; vel_ref_in: the caller's reference speed, used where has_ref; pid: the state before the
// call; piece, piece_la: spline piece hints (in: where to start the lookups; out: the pieces used).
__device__ __forceinline__ vanilla_decision vanilla_decide(const lmpc_spline_view& T, const lmpc_vehicle& veh, const lmpc_vanilla_config& c,
                                                           const double* x, bool has_ref, double vel_ref_in, double speed_scale,
                                                           const vanilla_pid& pid, int& piece, int& piece_la) {
#pragma clang fp contract(off)
  const double s = x[0];
  // current pose: frenet_to_global(s, e_y, e_psi) (racing_trajectory.cpp:122-186, as lmpc_track_to_global_kernel)
  const track_point r = track_eval(T, s, piece);
  const double yaw0 = atan2(r.dy, r.dx);
  const double px = r.x - sin(yaw0) * x[1];
  const double py = r.y + cos(yaw0) * x[1];
  const double yaw = track_align_yaw(yaw0 + x[2], 0.0);
  // pure pursuit target (:68-78): the centre line at the lookahead abscissa, zero offset
  const double v = hypot(x[3], x[4]);
  const double la = vanilla_clamp(v * c.lookahead_speed_ratio, c.min_lookahead_distance, c.max_lookahead_distance);
  const double s_la = track_mod(s + la, T.L);
  const track_point q = track_eval(T, s_la, piece_la);
  // steering (:81-89)
  const double dir = atan2(q.y - py, q.x - px);
  const double d = dir - yaw;
  const double alpha = atan2(sin(d), cos(d));
  const double delta = atan(2.0 * veh.l * sin(alpha) / la);
  double steer = vanilla_clamp(delta, -veh.max_steer, veh.max_steer);
  // reference speed: the caller's, or the velocity interpolant at the car's abscissa (vanilla_controller_node.cpp:104) times speed_scale
  double vel_ref = vel_ref_in;
  if (!has_ref) {
    const double h = track_mod(s, T.L) - T.breaks[piece];
    vel_ref = poly0(track_load(T.coef, piece, 2), h) * speed_scale;
  }
  // PidController::update(vel_ref - v, dt)
  const double e = vel_ref - v;
  vanilla_pid np = pid;
  double cmd;
  if (isnan(e)) {
    cmd = NAN;
  } else {
    np.last_error = pid.error;
    np.error = e;
    np.integral = vanilla_clamp(pid.integral + e * c.dt, c.min_i, c.max_i);
    const double dt_error = (np.error - np.last_error) / c.dt;
    cmd = e * c.k_p + np.integral * c.k_i + dt_error * c.k_d;
    if (cmd <= c.min_cmd)
      cmd = c.min_cmd;
    else if (cmd >= c.max_cmd)
      cmd = c.max_cmd;
  }
  // force (:94-105)
  const double aero = 0.5 * veh.rho * veh.Af * veh.cd * v * v;
  const double down = aero * (veh.cl_f + veh.cl_r);
  const double roll = veh.fr * (veh.m * LMPC_VANILLA_GRAVITY + down);
  double F = veh.m * cmd + roll + aero;
  // an abscissa beyond LMPC_VANILLA_LAPS_MAX laps: align_abscissa would wrap it to something finite; refuse it instead
  if (!(fabs(s) <= LMPC_VANILLA_LAPS_MAX * T.L)) F = steer = NAN;
  vanilla_decision o;
  o.FD = F > 0.0 ? F : 0.0;  // (a NaN force goes to FB, as `ctrl_force > 0.0` sends it upstream)
  o.FB = F > 0.0 ? 0.0 : F;
  o.steer = steer;
  const double ua = fabs(o.FD) > fabs(o.FB) ? o.FD : o.FB;  // the node's fold (vanilla_controller_node.cpp:118-122)
  o.um0 = ua * c.force_to_lon;
  o.pid = np;
  o.finite = isfinite(o.FD) && isfinite(o.FB) && isfinite(steer);
  return o;
}

__global__ __launch_bounds__(64) void lmpc_vanilla_solve_kernel(lmpc_spline_view T, lmpc_vehicle veh, lmpc_vanilla_store st, int B,
                                                                const double* __restrict__ x_ic, const double* __restrict__ vel_ref,
                                                                double speed_scale, double* __restrict__ u_out,
                                                                double* __restrict__ u_model, int* __restrict__ flags) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const size_t Bz = (size_t)B;
  double x[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) x[k] = x_ic[k * Bz + b];
  const vanilla_pid pid = {st.pid[b], st.pid[Bz + b], st.pid[2 * Bz + b]};
  int piece = 0, piece_la = 0;
  const vanilla_decision o = vanilla_decide(T, veh, st.cfg, x, vel_ref != nullptr, vel_ref ? vel_ref[b] : 0.0, speed_scale, pid, piece, piece_la);
  u_out[b] = o.FD;
  u_out[Bz + b] = o.FB;
  u_out[2 * Bz + b] = o.steer;
  if (u_model) {
    u_model[b] = o.um0;
    u_model[Bz + b] = o.steer;
  }
  if (flags) flags[b] = o.finite ? 0 : LMPC_VANILLA_FLAG_NOT_FINITE;
  if (o.finite) {
    st.pid[b] = o.pid.integral;
    st.pid[Bz + b] = o.pid.error;
    st.pid[2 * Bz + b] = o.pid.last_error;
  }
}

// The plant (lmpc_plant_kernel): nsub sub-steps of dt_sim with the input held, x_io [6] in place.  Kept OUT OF LINE and in the form of
// lmpc_plant_kernel's body -- vehicle and table by value, the state loaded once and stored once.  Which products the compiler
// contracts into FMAs inside the inlined model depends on the code around it, and a rollout is held against one
// lmpc_plant_step_batch per period (closed_loop.run_vanilla fused against unfused; the fleet recorder's rings are compared bit for
// bit).  Measured on 67 BARC and 67 IAC cars, one period: inlined into the period loop a quarter of the cars differed from
// lmpc_plant_kernel by an ulp in some component; out of line with the vehicle by reference one IAC car still did; in this form none
// does, and 700 periods of 67 cars record identical laps.  That is a property of this compiler on this source, not a guarantee:
// tests/test_gpu_vanilla.py holds it.  The call costs 284 bytes of scratch per lane and nothing measurable beside the 4 nsub model
// evaluations it makes.
__device__ __noinline__ void vanilla_plant(lmpc_vehicle veh, lmpc_track trk, double* __restrict__ x_io, double u0, double u1, double dt_sim,
                                           int nsub) {
  // (the form of lmpc_plant_kernel's body: everything by value, the state loaded once and stored once)
  double x[6], xn[6];
  const double u[2] = {u0, u1};
#pragma unroll
  for (int k = 0; k < 6; ++k) x[k] = x_io[k];
  for (int j = 0; j < nsub; ++j) {
    if (fabs(x[3]) < 1e-6) x[3] = copysign(1e-6, x[3]);  // racing_simulator.cpp:99-102
    const double kap = track_lookup(trk.curvature, trk.M, trk.L, x[0]);
    lmpc_fd(veh, x, u, kap, dt_sim, xn);
    // align_abscissa(s, L/2, L): lmpc_utils/utils.hpp:35-41
    const double s1 = xn[0], s2 = trk.L / 2.0;
    const double kk = fabs(s2 - s1) + trk.L / 2.0;
    const double ll = kk - fmod(kk, trk.L);
    xn[0] = s1 + ll * ((s2 > s1) - (s2 < s1));
#pragma unroll
    for (int k = 0; k < 6; ++k) x[k] = xn[k];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) x_io[k] = x[k];
}

__global__ __launch_bounds__(64) void lmpc_vanilla_rollout_kernel(lmpc_spline_view T, lmpc_vehicle veh, lmpc_vanilla_store st, lmpc_track trk,
                                                                  int B, int periods, double dt_sim, int nsub, double speed_scale,
                                                                  lmpc_vanilla_rollout_io io) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const size_t Bz = (size_t)B, Pz = (size_t)periods;
  double x[6], xs[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) x[k] = io.x[k * Bz + b];
  vanilla_pid pid = {st.pid[b], st.pid[Bz + b], st.pid[2 * Bz + b]};
  // the accumulators continue from the caller's values, sample by sample: two launches of 32 periods leave the bits of one of 64
  double dist = io.distance ? io.distance[b] : 0.0, worst = io.worst_excess ? io.worst_excess[b] : -INFINITY;
  const double half_b = veh.b / 2.0;
  int piece = 0, piece_la = 0;  // carried from one period to the next: the car moves a fraction of a piece per period
  bool frozen = false;
#pragma unroll 1
  for (size_t p = 0; p < Pz; ++p) {
    if (!frozen) {
      const vanilla_decision o = vanilla_decide(T, veh, st.cfg, x, false, 0.0, speed_scale, pid, piece, piece_la);
      if (!o.finite) {
        frozen = true;
      } else {
        const double u[2] = {o.um0, o.steer};
#pragma unroll
        for (int k = 0; k < 6; ++k) xs[k] = x[k];
        vanilla_plant(veh, trk, xs, u[0], u[1], dt_sim, nsub);
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 6; ++k) ok = ok && isfinite(xs[k]);
        if (!ok) {
          frozen = true;  // the period is undone: x and the PID state stay as they were before it
        } else {
          if (io.X_log) {
#pragma unroll
            for (int k = 0; k < 6; ++k) io.X_log[(k * Pz + p) * Bz + b] = x[k];
          }
          if (io.U_log) {
            io.U_log[p * Bz + b] = u[0];
            io.U_log[(Pz + p) * Bz + b] = u[1];
          }
          if (io.k_log) io.k_log[p * Bz + b] = vanilla_lookup(trk.curvature, trk.M, trk.L, x[0]);
          // bookkeeping, as lmpc_loop_advance_kernel keeps it
          const double ds = xs[0] - x[0];
          dist += (ds < -trk.L / 2.0) ? ds + trk.L : ds;
          if (io.worst_excess) {
            const double bl = vanilla_lookup(trk.bound_left, trk.M, trk.L, x[0]), br = vanilla_lookup(trk.bound_right, trk.M, trk.L, x[0]);
            worst = fmax(worst, fmax(xs[1] + half_b - bl, br - (xs[1] - half_b)));
          }
#pragma unroll
          for (int k = 0; k < 6; ++k) x[k] = xs[k];
          pid = o.pid;
        }
      }
    }
    if (frozen) {
      if (io.X_log) {
#pragma unroll
        for (int k = 0; k < 6; ++k) io.X_log[(k * Pz + p) * Bz + b] = NAN;
      }
      if (io.U_log) {
        io.U_log[p * Bz + b] = NAN;
        io.U_log[(Pz + p) * Bz + b] = NAN;
      }
      if (io.k_log) io.k_log[p * Bz + b] = NAN;
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) io.x[k * Bz + b] = x[k];
  st.pid[b] = pid.integral;
  st.pid[Bz + b] = pid.error;
  st.pid[2 * Bz + b] = pid.last_error;
  if (io.distance) io.distance[b] = dist;
  if (io.worst_excess) io.worst_excess[b] = worst;
  if (io.flags) io.flags[b] = frozen ? LMPC_VANILLA_FLAG_NOT_FINITE : 0;
}

// The double-track plant of one period (lmpc_plant_dtrack_kernel: conversion on entry and exit, guard, lookup, Newton on gamma_y,
// wrap), OUT OF LINE in vanilla_plant's form -- vehicle and table by value, x_io [6] loaded once and stored once -- around the one
// text of lmpc_dtrack_dynamics.hip.h.  Out of line it is also the only code of the rollout that needs the model's registers.
__device__ __noinline__ void vanilla_plant_dtrack(lmpc_vehicle_dt veh, lmpc_track trk, double* __restrict__ x_io, double u0, double u1,
                                                  double dt_sim, int nsub) {
#define LMPC_VANILLA_XIO_(k) x_io[k]
  LMPC_DTRACK_STEP_CAR(veh, trk, LMPC_VANILLA_XIO_, u0, u1, dt_sim, nsub)
#undef LMPC_VANILLA_XIO_
  (void)gamma_first;
}

// lmpc_vanilla_rollout_kernel with car b on a plant of its own and its recorder fed inside the period loop
// (include/lmpc_hip_vanilla_fleet.h).  PLANT: LMPC_VANILLA_PLANT_HANDLE steps with `veh` (vanilla_plant as lmpc_vanilla_rollout_kernel
// calls it), _CARS with vehicle b of the car table (loaded once, the same out-of-line function), _DTRACK with four-wheel vehicle b
// of the double-track table.  REC: a live period -- finite decision, finite state after the plant -- hands (x_p, input, curvature,
// (period0 + p) dt) to lmpc_fleet_record_car; the input is the one applied from x_p, or with fx.arrived the one that led to it.
// The decision reads `veh`, the handle's vehicle, whatever the plant.  The text of the period loop is lmpc_vanilla_rollout_kernel's.
template <int PLANT, bool REC>
__global__ __launch_bounds__(64) void lmpc_vanilla_fleet_kernel(lmpc_spline_view T, lmpc_vehicle veh, lmpc_vanilla_store st, lmpc_track trk,
                                                                int B, int periods, double dt_sim, int nsub, double speed_scale,
                                                                lmpc_vanilla_rollout_io io, lmpc_vanilla_fleet_io fx, lmpc_fleet_store fs) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const size_t Bz = (size_t)B, Pz = (size_t)periods;
  lmpc_vehicle car;
  lmpc_vehicle_dt car_dt;
  if constexpr (PLANT == LMPC_VANILLA_PLANT_CARS) lmpc_car_vehicle(fx.table, B, b, car);
  if constexpr (PLANT == LMPC_VANILLA_PLANT_DTRACK) dtrack_vehicle(fx.table, B, b, car_dt);
  double x[6], xs[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) x[k] = io.x[k * Bz + b];
  vanilla_pid pid = {st.pid[b], st.pid[Bz + b], st.pid[2 * Bz + b]};
  // the accumulators continue from the caller's values, sample by sample: two launches of 32 periods leave the bits of one of 64
  double dist = io.distance ? io.distance[b] : 0.0, worst = io.worst_excess ? io.worst_excess[b] : -INFINITY;
  const double half_b = veh.b / 2.0;
  int piece = 0, piece_la = 0;  // carried from one period to the next: the car moves a fraction of a piece per period
  bool frozen = false, moved = false;
  double up0 = 0.0, up1 = 0.0;  // the last input applied; on entry the caller's (read where the recorder takes it)
  if (REC && fx.arrived) {
    up0 = fx.u_prev[b];
    up1 = fx.u_prev[Bz + b];
  }
#pragma unroll 1
  for (size_t p = 0; p < Pz; ++p) {
    if (!frozen) {
      const vanilla_decision o = vanilla_decide(T, veh, st.cfg, x, false, 0.0, speed_scale, pid, piece, piece_la);
      if (!o.finite) {
        frozen = true;
      } else {
        const double u[2] = {o.um0, o.steer};
#pragma unroll
        for (int k = 0; k < 6; ++k) xs[k] = x[k];
        if constexpr (PLANT == LMPC_VANILLA_PLANT_HANDLE) vanilla_plant(veh, trk, xs, u[0], u[1], dt_sim, nsub);
        if constexpr (PLANT == LMPC_VANILLA_PLANT_CARS) vanilla_plant(car, trk, xs, u[0], u[1], dt_sim, nsub);
        if constexpr (PLANT == LMPC_VANILLA_PLANT_DTRACK) vanilla_plant_dtrack(car_dt, trk, xs, u[0], u[1], dt_sim, nsub);
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 6; ++k) ok = ok && isfinite(xs[k]);
        if (!ok) {
          frozen = true;  // the period is undone: x and the PID state stay as they were before it
        } else {
          if (io.X_log) {
#pragma unroll
            for (int k = 0; k < 6; ++k) io.X_log[(k * Pz + p) * Bz + b] = x[k];
          }
          if (io.U_log) {
            io.U_log[p * Bz + b] = u[0];
            io.U_log[(Pz + p) * Bz + b] = u[1];
          }
          if (io.k_log || REC) {
            const double kap = vanilla_lookup(trk.curvature, trk.M, trk.L, x[0]);
            if (io.k_log) io.k_log[p * Bz + b] = kap;
            if constexpr (REC) {
              const double t = (double)(fx.period0 + (long long)p) * fx.dt;
              lmpc_fleet_record_car(fs, b, x, fx.arrived ? up0 : u[0], fx.arrived ? up1 : u[1], kap, t, trk.L);
            }
          }
          up0 = u[0];
          up1 = u[1];
          moved = true;
          // bookkeeping, as lmpc_loop_advance_kernel keeps it
          const double ds = xs[0] - x[0];
          dist += (ds < -trk.L / 2.0) ? ds + trk.L : ds;
          if (io.worst_excess) {
            const double bl = vanilla_lookup(trk.bound_left, trk.M, trk.L, x[0]), br = vanilla_lookup(trk.bound_right, trk.M, trk.L, x[0]);
            worst = fmax(worst, fmax(xs[1] + half_b - bl, br - (xs[1] - half_b)));
          }
#pragma unroll
          for (int k = 0; k < 6; ++k) x[k] = xs[k];
          pid = o.pid;
        }
      }
    }
    if (frozen) {
      if (io.X_log) {
#pragma unroll
        for (int k = 0; k < 6; ++k) io.X_log[(k * Pz + p) * Bz + b] = NAN;
      }
      if (io.U_log) {
        io.U_log[p * Bz + b] = NAN;
        io.U_log[(Pz + p) * Bz + b] = NAN;
      }
      if (io.k_log) io.k_log[p * Bz + b] = NAN;
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) io.x[k * Bz + b] = x[k];
  st.pid[b] = pid.integral;
  st.pid[Bz + b] = pid.error;
  st.pid[2 * Bz + b] = pid.last_error;
  if (fx.u_prev && moved) {  // (a car frozen in period 0 applied nothing: its u_prev stays)
    fx.u_prev[b] = up0;
    fx.u_prev[Bz + b] = up1;
  }
  if (io.distance) io.distance[b] = dist;
  if (io.worst_excess) io.worst_excess[b] = worst;
  if (io.flags) io.flags[b] = frozen ? LMPC_VANILLA_FLAG_NOT_FINITE : 0;
}

}  // namespace

hipError_t lmpc_vanilla_launch_solve(hipStream_t stream, const lmpc_vanilla_store& st, const lmpc_vehicle& veh, const lmpc_spline_view& track,
                                     int batch, const double* x_ic, const double* vel_ref, double speed_scale, double* u_out, double* u_model,
                                     int* flags) {
  hipLaunchKernelGGL(lmpc_vanilla_solve_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, stream, track, veh, st, batch, x_ic, vel_ref,
                     speed_scale, u_out, u_model, flags);
  return hipGetLastError();
}

hipError_t lmpc_vanilla_launch_rollout(hipStream_t stream, const lmpc_vanilla_store& st, const lmpc_vehicle& veh, const lmpc_spline_view& track,
                                       const lmpc_track& table, int batch, int periods, double dt_sim, int n_sub, double speed_scale,
                                       const lmpc_vanilla_rollout_io& io) {
  hipLaunchKernelGGL(lmpc_vanilla_rollout_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, stream, track, veh, st, table, batch, periods,
                     dt_sim, n_sub, speed_scale, io);
  return hipGetLastError();
}

hipError_t lmpc_vanilla_launch_fleet(hipStream_t stream, const lmpc_vanilla_store& st, const lmpc_vehicle& veh, const lmpc_spline_view& track,
                                     const lmpc_track& table, int batch, int periods, double dt_sim, int n_sub, double speed_scale,
                                     const lmpc_vanilla_rollout_io& io, int plant, bool record, const lmpc_vanilla_fleet_io& fx,
                                     const lmpc_fleet_store& fs) {
  const dim3 grid((unsigned)((batch + 63) / 64)), block(64);
#define LMPC_VANILLA_FLEET_LAUNCH_(PLANT, REC)                                                                                        \
  hipLaunchKernelGGL((lmpc_vanilla_fleet_kernel<PLANT, REC>), grid, block, 0, stream, track, veh, st, table, batch, periods, dt_sim, n_sub, \
                     speed_scale, io, fx, fs)
  switch (plant * 2 + (record ? 1 : 0)) {
    case LMPC_VANILLA_PLANT_HANDLE * 2: LMPC_VANILLA_FLEET_LAUNCH_(LMPC_VANILLA_PLANT_HANDLE, false); break;
    case LMPC_VANILLA_PLANT_HANDLE * 2 + 1: LMPC_VANILLA_FLEET_LAUNCH_(LMPC_VANILLA_PLANT_HANDLE, true); break;
    case LMPC_VANILLA_PLANT_CARS * 2: LMPC_VANILLA_FLEET_LAUNCH_(LMPC_VANILLA_PLANT_CARS, false); break;
    case LMPC_VANILLA_PLANT_CARS * 2 + 1: LMPC_VANILLA_FLEET_LAUNCH_(LMPC_VANILLA_PLANT_CARS, true); break;
    case LMPC_VANILLA_PLANT_DTRACK * 2: LMPC_VANILLA_FLEET_LAUNCH_(LMPC_VANILLA_PLANT_DTRACK, false); break;
    case LMPC_VANILLA_PLANT_DTRACK * 2 + 1: LMPC_VANILLA_FLEET_LAUNCH_(LMPC_VANILLA_PLANT_DTRACK, true); break;
    default: return hipErrorInvalidValue;
  }
#undef LMPC_VANILLA_FLEET_LAUNCH_
  return hipGetLastError();
}
