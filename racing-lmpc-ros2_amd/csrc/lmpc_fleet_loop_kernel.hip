// lmpc_fleet_loop_kernel.hip -- everything between two solves of a fleet LMPC period in one launch (lmpc_fleet_loop_advance_batch):
// closed_loop.run_lmpc_fleet's loop body from the solve of period k to just before the solve of period k + 1.  Per car, in order:
//   1 the solution of the controller the car drives with (phase 0: tracking, 1: learning), 2 the input applied and the plant,
//   3 the next references (lmpc_loop_advance_kernel's three routes, with the phase's speed triple), 4 x_ic, 5 the car's recorder and
//   ring (lmpc_fleet_ss_record_kernel's body), 6 the lap book, 7 the phase, 8 the next k-NN query point.
// Steps 2, 3 and 5 are the text of lmpc_loop_steps.hip.h, the same the kernels they come from are made of.  On four-wheel cars
// (lmpc_fleet_loop_advance_dtrack_batch, include/lmpc_hip_fleet_dtrack.h) step 2's plant is the text of lmpc_dtrack_dynamics.hip.h.
//
// Shape: lmpc_loop_advance_kernel's.  A workgroup is 64 cars (the lanes) x lmpc_loop_waves waves; wave 0 is the car -- input, plant,
// books, recorder, phase, query -- and the waves share the knots of a shifted solution.  A failed car is wave 0's alone.
//
// Two hazards, and the route taken:
//   - phase[b] is read by every wave (it selects the solution to shift) and written by wave 0 in step 7.  Every wave reads it FIRST,
//     then the workgroup meets at the kernel's one barrier, which is the first statement after that load: no return, no branch on
//     lane or wave stands in front of it, so every lane of every wave reaches it (cars past the batch included).  No LDS.
//   - step 8 needs the new state (wave 0's) and the last knot of the new X_ref.  There is NO barrier for that: wave 0 owns the last
//     knot.  The waves share knots 0 .. N - 2 (wave w: w, w + W, ...), and wave 0 then makes knot N - 1 itself -- the one-step
//     rollout -- so the query is formed from the registers the knot was stored from and equals the formula on the X_ref this call
//     wrote, bit for bit.  For a failed car wave 0 walks all knots anyway and ends holding the last.  Behind the barrier the waves
//     never meet again, so the early returns (cars past the batch, failed cars' other waves, waves other than 0 when their knots are
//     done) cannot hang anything.
// Ordinary vector loads and stores, and two vector atomics (the counters).
#include <hip/hip_runtime.h>

#include "lmpc_cars.h"
#include "lmpc_dtrack_dynamics.hip.h"
#include "lmpc_fleet_loop.h"
#include "lmpc_loop_steps.hip.h"

// The three rollouts, OUT OF LINE and in the form of the bodies of lmpc_plant_kernel, lmpc_prepare_kernel and lmpc_shift_kernel --
// vehicle, table and arrays by value, the scratch arrays their own -- around the one text of lmpc_loop_steps.hip.h.  A call's code
// does not depend on its caller, so the contraction inside the model is the same whatever this kernel does around it (the vanilla
// rollout's plant is kept out of line for the same reason), and by instruction mix it is that of the three kernels the results are
// held to (tests/test_gpu_fleet_loop.py).  The price: 848 bytes of scratch per lane and 19 spilled VGPRs for the kernel.  The two
// failed-car routes are rare; fleet_loop_plant is NOT -- every car's wave 0 calls it every period, with its state in memory across
// the call.  Measured, 4096 cars: 37.8 us per launch, against 41.8 + 15.5 + 4.8 + 4.6 us for the shift, plant, record and stats
// kernels it replaces and 3.8 % of a period's GPU time (profiles/fleet_lmpc_fused.md).  Inlining the plant again would take the
// scratch off the common path; it is worth doing only with a GPU run that shows lmpc_plant_kernel's bits still met on every car.
struct lmpc_last_knot {
  double s, ey;
};
__device__ __noinline__ void fleet_loop_plant(lmpc_vehicle veh, lmpc_track trk, double* __restrict__ x_io, double u0, double u1, double dt_sim,
                                              int nsub) {
  double x[6], xn[6];
  const double u[2] = {u0, u1};
#pragma unroll
  for (int k = 0; k < 6; ++k) x[k] = x_io[k];
  LMPC_PLANT_SUBSTEPS(veh, trk, x, u, dt_sim, nsub, xn)
#pragma unroll
  for (int k = 0; k < 6; ++k) x_io[k] = x[k];
}
__device__ __noinline__ lmpc_last_knot fleet_loop_cold_restart(lmpc_vehicle veh, lmpc_track trk, lmpc_ref_arrays r, int b, int B, int N, double x0,
                                                               double x1, double x2, double x3, double x4, double x5, double dt, double d,
                                                               double speed_scale, double speed_limit) {
  double x[6] = {x0, x1, x2, x3, x4, x5}, xn[6];
  LMPC_CAR_COLD_RESTART(veh, trk, r, b, B, N, x, xn, dt, d, speed_scale, speed_limit)
  return {x[0], x[1]};
}
__device__ __noinline__ lmpc_last_knot fleet_loop_shift_in_place(lmpc_vehicle veh, lmpc_track trk, lmpc_ref_arrays r, int b, int B, int N, double dt,
                                                                 double d, double speed_scale, double speed_limit) {
  double x[6], xn[6], u[2] = {0.0, 0.0};
  LMPC_CAR_SHIFT_IN_PLACE(veh, trk, r, b, B, N, x, xn, u, dt, d, speed_scale, speed_limit)
  return {x[0], x[1]};
}

// The double-track plant of one period (lmpc_plant_dtrack_kernel: conversion on entry and exit, guard, lookup, Newton on gamma_y,
// wrap), OUT OF LINE in vanilla_plant_dtrack's form (lmpc_vanilla_kernel.hip) -- vehicle and table by value, x_io [6] loaded once and
// stored once -- around the one text of lmpc_dtrack_dynamics.hip.h.  Out of line it is the only code of the kernel that needs the
// four-wheel model's registers: none of them is live across steps 3 to 8.  Returns the gamma_y solved in the first evaluation of the
// dynamics of the last sub-step.
__device__ __noinline__ double fleet_loop_plant_dtrack(lmpc_vehicle_dt veh, lmpc_track trk, double* __restrict__ x_io, double u0, double u1,
                                                       double dt_sim, int nsub) {
#define LMPC_FLEET_LOOP_XIO_(k) x_io[k]
  LMPC_DTRACK_STEP_CAR(veh, trk, LMPC_FLEET_LOOP_XIO_, u0, u1, dt_sim, nsub)
#undef LMPC_FLEET_LOOP_XIO_
  return gamma_first;
}

// One text, three instantiations (lmpc_fleet_loop.h names them).  _HANDLE is the kernel as it always was: io.plant blanked by the
// host, every car's plant K.plant.  _CARS: io.plant is the DEVICE car table of csrc/lmpc_cars.h (the host puts it there; a table of
// st.B cars), and step 2 loads car b's vehicle from it and hands that to the same fleet_loop_plant.  _DTRACK: step 2 loads car b's
// four-wheel vehicle from K.table, the double-track table of csrc/lmpc_dtrack.h, and hands it to fleet_loop_plant_dtrack; K.gamma_y,
// when not null, receives what that returns.  A kernel each and not a run-time branch in the first, and the kernel itself the
// template, not a wrapper around an inlined body: so instantiated, _HANDLE is the instruction stream, the 256 VGPRs and the 848
// bytes of scratch it had as a plain kernel (compared on the compiler's assembly; behind a wrapper its scratch grew to 928 bytes),
// which is what tests/test_gpu_fleet_loop.py and profiles/fleet_lmpc_fused.md hold it to; profiles/fleet_dtrack_fused.md has the
// same comparison with the third instantiation beside the two.
// Everything but step 2's vehicle is the same in all: the reference rollouts, the cold restart, the in-place shift and the body
// width of worst_excess use the handle's vehicle K.veh -- the controllers share one model.
template <int PLANT>
__global__ __launch_bounds__(64 * lmpc_loop_waves) void lmpc_fleet_loop_kernel(lmpc_fleet_loop_consts_of<PLANT> K, lmpc_fleet_store st,
                                                                               lmpc_track trk, lmpc_fleet_loop io) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * 64 + lane;
  const int B = st.B, N = K.N, NS = N - 1;
  const bool live = b < B;
  const int sel = (live && io.phase[b] != 0) ? 1 : 0;  // the phase as it stands at entry
  __syncthreads();  // every wave has read phase[b] before wave 0 may write it (see the head of the file)
  if (!live) return;
  const bool head_only = !io.X_trk && !io.X_lrn;  // (the host has checked: triples are whole or absent)
  if (head_only && w != 0) return;
  const lmpc_ref_arrays refs{io.X_ref, io.U_ref, io.T_ref, io.bound_left, io.bound_right, io.curvatures, io.vel_ref};
  double x[6], u[2], last_s, last_ey;  // wave 0: the car's state, the input applied, the last knot of the new reference
  if (head_only) {
#pragma unroll
    for (int k = 0; k < 6; ++k) x[k] = io.x[(size_t)k * B + b];
#pragma unroll
    for (int k = 0; k < 2; ++k) u[k] = io.u_prev[(size_t)k * B + b];
    last_s = io.X_ref[(size_t)(0 * N + NS) * B + b];
    last_ey = io.X_ref[(size_t)(1 * N + NS) * B + b];
  } else {
    // ---- 1 the solution ----
    const double* X_sol = sel ? io.X_lrn : io.X_trk;
    const double* U_sol = sel ? io.U_lrn : io.U_trk;
    const int* status = sel ? io.status_lrn : io.status_trk;
    const bool ok = X_sol && status[b] == 0;  // a car whose controller did not run counts as a failed solve
    const double speed_scale = io.speed_scale[sel], speed_limit = io.speed_limit[sel], d = io.max_vel_ref_diff[sel];
    if (w == 0) {
      // ---- 2 the input applied, the plant (lmpc_loop_advance_kernel) ----
#pragma unroll
      for (int k = 0; k < 2; ++k) u[k] = ok ? U_sol[(size_t)(k * NS) * B + b] : io.U_ref[(size_t)(k * NS) * B + b];
#pragma unroll
      for (int k = 0; k < 6; ++k) x[k] = io.x[(size_t)k * B + b];
      const double s_before = x[0];
      if constexpr (PLANT == LMPC_FLEET_PLANT_DTRACK) {
        lmpc_vehicle_dt car;
        dtrack_vehicle(K.table, B, b, car);
        const double gamma_first = fleet_loop_plant_dtrack(car, trk, x, u[0], u[1], io.dt_sim, io.n_sub);
        if (K.gamma_y) K.gamma_y[b] = gamma_first;
      } else if constexpr (PLANT == LMPC_FLEET_PLANT_CARS) {
        lmpc_vehicle car;
        lmpc_car_vehicle(reinterpret_cast<const double*>(io.plant), B, b, car);
        fleet_loop_plant(car, trk, x, u[0], u[1], io.dt_sim, io.n_sub);
      } else {
        fleet_loop_plant(K.plant, trk, x, u[0], u[1], io.dt_sim, io.n_sub);
      }
#pragma unroll
      for (int k = 0; k < 6; ++k) io.x[(size_t)k * B + b] = x[k];
#pragma unroll
      for (int k = 0; k < 2; ++k) io.u_prev[(size_t)k * B + b] = u[k];
      if (io.distance) {
        const double ds = x[0] - s_before;
        io.distance[b] += (ds < -trk.L / 2.0) ? ds + trk.L : ds;
      }
      if (io.worst_excess) {
        const double half_b = K.veh.b / 2.0;
        const double exc = fmax(x[1] + half_b - io.bound_left[b], io.bound_right[b] - (x[1] - half_b));  // (knot 0 of the period just driven)
        io.worst_excess[b] = fmax(io.worst_excess[b], exc);
      }
      if (io.n_fail && !ok) io.n_fail[b] += 1;
    }
    // ---- 3 the next references; the rollouts use the handle's vehicle ----
    if (!ok) {
      if (w != 0) return;
      const lmpc_last_knot l = io.restart_failed
                                   ? fleet_loop_cold_restart(K.veh, trk, refs, b, B, N, x[0], x[1], x[2], x[3], x[4], x[5], io.dt, d, speed_scale, speed_limit)
                                   : fleet_loop_shift_in_place(K.veh, trk, refs, b, B, N, io.dt, d, speed_scale, speed_limit);
      last_s = l.s;
      last_ey = l.ey;
    } else {
      double xk[6];
      for (int i = w; i < NS; i += lmpc_loop_waves)
        lmpc_car_shift_knot(K.veh, trk, refs, b, B, N, i, X_sol, U_sol, xk, io.dt, d, speed_scale, speed_limit);
      if (w != 0) return;
      lmpc_car_shift_knot(K.veh, trk, refs, b, B, N, NS, X_sol, U_sol, xk, io.dt, d, speed_scale, speed_limit);
      last_s = xk[0];
      last_ey = xk[1];
    }
  }
  // ---- wave 0 from here on ----
  // 4 x_ic: the measured state, projected onto the state box for a car that drove this period with the learning controller
#pragma unroll
  for (int k = 0; k < 6; ++k) io.x_ic[(size_t)k * B + b] = sel ? fmin(fmax(x[k], K.x_min[k]), K.x_max[k]) : x[k];
  // 5 the recorder and the ring
  const int count_before = st.lap_count[b];
  const bool crossed = lmpc_fleet_record_car(st, b, x, u[0], u[1], track_lookup(trk.curvature, trk.M, trk.L, x[0]), io.t, trk.L);
  // 6 the lap book: slot i of car b is its i-th closed lap (the first crossing closes the discarded partial lap)
  if (crossed && count_before >= 1) {
    if (count_before <= io.n_rec) {
      const int dn = st.dur_n[b];  // (what lmpc_fleet_ss_stats_kernel reports as the last lap time)
      io.lap_time[(size_t)(count_before - 1) * B + b] = dn > 0 ? st.dur[(size_t)b * LMPC_FLEET_DUR + (dn - 1) % LMPC_FLEET_DUR] : 0.0;
      io.lap_kind[(size_t)(count_before - 1) * B + b] = sel;
    }
    if (sel) {
      const int nl = io.n_learn[b] + 1;
      io.n_learn[b] = nl;
      if (nl == io.learn_laps) atomicAdd(io.counters + 1, 1);
    }
  }
  // 7 the phase, after the lap's kind was noted
  if (io.switch_phase && !sel && st.cnt[b] >= io.warm_laps) {
    io.phase[b] = 1;
    atomicAdd(io.counters, 1);
  }
  // 8 the next query point: the last knot of the reference, its abscissa aligned with the car's (racing_mpc.cpp:219-223,249-254)
  const double ds = x[0] - last_s;
  const double kk = fabs(ds) + trk.L / 2.0;
  const double ll = kk - fmod(kk, trk.L);
  io.query[b] = last_s + ll * (double)((ds > 0.0) - (ds < 0.0));  // (ll is a whole number of laps times +-1 or 0: the product is exact)
  io.query[(size_t)B + b] = last_ey;
}

template __global__ void lmpc_fleet_loop_kernel<LMPC_FLEET_PLANT_HANDLE>(lmpc_fleet_loop_consts, lmpc_fleet_store, lmpc_track, lmpc_fleet_loop);
template __global__ void lmpc_fleet_loop_kernel<LMPC_FLEET_PLANT_CARS>(lmpc_fleet_loop_consts, lmpc_fleet_store, lmpc_track, lmpc_fleet_loop);
template __global__ void lmpc_fleet_loop_kernel<LMPC_FLEET_PLANT_DTRACK>(lmpc_fleet_loop_consts_dt, lmpc_fleet_store, lmpc_track, lmpc_fleet_loop);
