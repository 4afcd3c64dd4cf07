// lmpc_loop_steps.hip.h -- what one car does between two solves, as the kernels that fuse those steps share it: the plant's
// sub-steps, the reference sampling at a knot, one knot of a shifted solution, the in-place shift of the old plan, the cold restart
// (lmpc_loop_advance_kernel in lmpc_prep_kernels.hip; lmpc_fleet_loop_kernel.hip), and the body of SafeSetRecorder::step on a car of
// an lmpc_fleet_store (lmpc_fleet_ss_record_kernel in lmpc_fleet_ss_kernel.hip; lmpc_fleet_loop_kernel.hip).  One text for each
// step: the kernels that share a step compute it with the same operations in the same order.
#ifndef LMPC_LOOP_STEPS_HIP_H_
#define LMPC_LOOP_STEPS_HIP_H_

#include <hip/hip_runtime.h>

#include "lmpc_device.h"
#include "lmpc_dynamics.hip.h"
#include "lmpc_fleet_ss.h"
#include "lmpc_track.hip.h"

// waves of 64 cars in a workgroup of lmpc_loop_advance_kernel and lmpc_fleet_loop_kernel
constexpr int lmpc_loop_waves = 8;  // (measured on the closed loop at 4 / 8 / 16, profiles/r05_tail_ab.txt: 6.49 / 6.53 / 6.36 M car-steps/s at 4096 cars warm)

// the seven reference arrays of a batch, [field][knot][batch]; no __restrict__: the in-place shift reads what it writes
struct lmpc_ref_arrays {
  double* X;     // [6][N][B]
  double* U;     // [2][N-1][B]
  double* T;     // [N-1][B]
  double* bl;    // [N][B]
  double* br;    // [N][B]
  double* curv;  // [N][B]
  double* vref;  // [N][B]
};

// Reference sampling at one knot (racing_mpc_node.cpp:261-292): bounds, curvature, clamped velocity reference.
__device__ __forceinline__ void sample_refs(const lmpc_track& trk, double s, double cur, double d, double speed_scale,
                                            double speed_limit, double& bl, double& br, double& kap, double& vr_out) {
  kap = track_lookup(trk.curvature, trk.M, trk.L, s);
  bl = track_lookup(trk.bound_left, trk.M, trk.L, s);
  br = track_lookup(trk.bound_right, trk.M, trk.L, s);
  const double vr = track_lookup(trk.vel, trk.M, trk.L, s) * speed_scale;
  const double lim = fmin(fmax(speed_limit, cur - d), cur + d);       // :273-275
  const double clipped = fmin(fmax(vr, cur - d), cur + d);
  vr_out = (vr > 0.0) ? fmin(clipped, lim) : lim;                     // :276-285
}

// knot i of car b: the state, and the references sampled at its abscissa
__device__ __forceinline__ void lmpc_store_knot(const lmpc_track& trk, const lmpc_ref_arrays& r, int b, int B, int N, int i, const double* x,
                                                double d, double speed_scale, double speed_limit, double& kap) {
#pragma unroll
  for (int k = 0; k < 6; ++k) r.X[(size_t)(k * N + i) * B + b] = x[k];
  double b_l, b_r, vr;
  sample_refs(trk, x[0], x[3], d, speed_scale, speed_limit, b_l, b_r, kap, vr);
  r.bl[(size_t)i * B + b] = b_l;
  r.br[(size_t)i * B + b] = b_r;
  r.curv[(size_t)i * B + b] = kap;
  r.vref[(size_t)i * B + b] = vr;
}

// The three rollouts of a car -- the plant, the cold restart, the in-place shift of the old plan -- are MACROS, not functions: one
// text, expanded where it is used.  Which products the compiler contracts into multiply-adds inside the inlined model depends on
// the code around it (the vanilla rollout), and these steps are held, bit for bit, to lmpc_plant_kernel,
// lmpc_prepare_kernel and lmpc_shift_kernel.  Measured: behind __forceinline__ functions lmpc_loop_advance_kernel fused twelve more
// multiply-adds than it had (any two of the three as functions left it alone), and the in-place shift as a function met
// lmpc_shift_kernel's instruction mix neither inline nor out of line, whether its scratch arrays were its own or the caller's.
// Expanded, lmpc_loop_advance_kernel is the text it always was, and lmpc_fleet_loop_kernel.hip wraps each expansion in an
// out-of-line function whose code does not depend on its caller.  x [6], xn [6] (one model step's result), u [2]: the caller's arrays.
// THE TRIPWIRE: an edit to these macros, to the code around an expansion or to lmpc_dynamics.hip.h can move the contraction again.
// What fails then: tests/test_gpu_loop.py::test_one_call_is_the_composition_of_the_entry_points_it_replaces (lmpc_loop_advance_kernel:
// the plant's state, every knot of a failed car) and tests/test_gpu_fleet_loop.py::test_one_call_is_the_composition_of_what_it_replaces
// (lmpc_fleet_loop_kernel: the same, "failed cars' last knot" first), both torch.equal against the three stand-alone kernels.
// The macros declare locals of their own -- j, i, k, kap, s1, s2, kk, ll, u0, src -- inside their braces; keep those names out of
// the arguments.

// RacingSimulator::step (racing_simulator.cpp:46-69,97-112): nsub sub-steps of dt_sim with the input held, the |vx| guard
// (:99-102), the table curvature at the current abscissa, the abscissa wrapped by align_abscissa(s, L/2, L).  x in place.
#define LMPC_PLANT_SUBSTEPS(veh, trk, x, u, dt_sim, nsub, xn)                                  \
  for (int j = 0; j < nsub; ++j) {                                                             \
    if (fabs(x[3]) < 1e-6) x[3] = copysign(1e-6, x[3]);                                        \
    const double kap = track_lookup(trk.curvature, trk.M, trk.L, x[0]);                        \
    lmpc_fd(veh, x, u, kap, dt_sim, xn);                                                       \
    const double s1 = xn[0], s2 = trk.L / 2.0;                                                 \
    const double kk = fabs(s2 - s1) + trk.L / 2.0;                                             \
    const double ll = kk - fmod(kk, trk.L);                                                    \
    xn[0] = s1 + ll * ((s2 > s1) - (s2 < s1));                                                 \
    _Pragma("unroll") for (int k = 0; k < 6; ++k) x[k] = xn[k];                                \
  }

// cold start of car b at state x (lmpc_prepare_kernel): zero-input rollout, references sampled along it into r (an
// lmpc_ref_arrays).  x is rolled along: behind the loop it is the last knot.
#define LMPC_CAR_COLD_RESTART(veh, trk, r, b, B, N, x, xn, dt, d, speed_scale, speed_limit)    \
  {                                                                                            \
    const double u0[2] = {1e-9, 1e-9};                                                         \
    for (int i = 0; i < N; ++i) {                                                              \
      double kap;                                                                              \
      lmpc_store_knot(trk, r, b, B, N, i, x, d, speed_scale, speed_limit, kap);                \
      if (i < N - 1) {                                                                         \
        r.U[(size_t)(0 * (N - 1) + i) * B + b] = u0[0];                                        \
        r.U[(size_t)(1 * (N - 1) + i) * B + b] = u0[1];                                        \
        r.T[(size_t)i * B + b] = dt;                                                           \
        lmpc_fd(veh, x, u0, kap, dt, xn);                                                      \
        _Pragma("unroll") for (int k = 0; k < 6; ++k) x[k] = xn[k];                            \
      }                                                                                        \
    }                                                                                          \
  }

// the plan a failed solve started from, shifted in place (lmpc_shift_kernel with X_old = X_ref): a thread reads knot i + 1 before
// it writes knot i + 1.  Behind the loop x is the last knot.
#define LMPC_CAR_SHIFT_IN_PLACE(veh, trk, r, b, B, N, x, xn, u, dt, d, speed_scale, speed_limit) \
  for (int i = 0; i < N; ++i) {                                                                \
    if (i < N - 1) {                                                                           \
      _Pragma("unroll") for (int k = 0; k < 6; ++k) x[k] = r.X[(size_t)(k * N + i + 1) * B + b]; \
    } else {                                                                                   \
      _Pragma("unroll") for (int k = 0; k < 6; ++k) x[k] = xn[k];                              \
    }                                                                                          \
    double kap;                                                                                \
    lmpc_store_knot(trk, r, b, B, N, i, x, d, speed_scale, speed_limit, kap);                  \
    if (i < N - 1) {                                                                           \
      const int src = (i < N - 2) ? i + 1 : N - 2; /* last input repeated */                   \
      _Pragma("unroll") for (int k = 0; k < 2; ++k) {                                          \
        u[k] = r.U[(size_t)(k * (N - 1) + src) * B + b];                                       \
        r.U[(size_t)(k * (N - 1) + i) * B + b] = u[k];                                         \
      }                                                                                        \
      r.T[(size_t)i * B + b] = dt;                                                             \
      if (i == N - 2) lmpc_fd(veh, x, u, kap, dt, xn);                                         \
    }                                                                                          \
  }

// knot i of the shifted solution of car b: knot i + 1 of the solution; the last one is rolled out from the solution's last knot
// with the repeated last input (racing_mpc_node.cpp:247-249).  Reads the solution only, writes the references.  x out: the knot.
__device__ __forceinline__ void lmpc_car_shift_knot(const lmpc_vehicle& veh, const lmpc_track& trk, const lmpc_ref_arrays& r, int b, int B,
                                                    int N, int i, const double* X_sol, const double* U_sol, double* x, double dt, double d,
                                                    double speed_scale, double speed_limit) {
  const int NS = N - 1;
  if (i < NS) {
#pragma unroll
    for (int k = 0; k < 6; ++k) x[k] = X_sol[(size_t)(k * N + i + 1) * B + b];
  } else {
    double xm[6], u[2];
#pragma unroll
    for (int k = 0; k < 6; ++k) xm[k] = X_sol[(size_t)(k * N + NS) * B + b];
#pragma unroll
    for (int k = 0; k < 2; ++k) u[k] = U_sol[(size_t)(k * NS + NS - 1) * B + b];
    const double kap_m = track_lookup(trk.curvature, trk.M, trk.L, xm[0]);
    lmpc_fd(veh, xm, u, kap_m, dt, x);
  }
  double kap;
  lmpc_store_knot(trk, r, b, B, N, i, x, d, speed_scale, speed_limit, kap);
  if (i < NS) {
    const int src = (i < NS - 1) ? i + 1 : NS - 1;
#pragma unroll
    for (int k = 0; k < 2; ++k) r.U[(size_t)(k * NS + i) * B + b] = U_sol[(size_t)(k * NS + src) * B + b];
    r.T[(size_t)i * B + b] = dt;
  }
}

// SafeSetRecorder::step (safe_set.cpp:278-322) + SafeSetManager::add_lap (:144-151) for car b of the store: the sample
// (x[6], u0, u1, k, t) on a track of length Lt.  Returns whether the sample crossed the start line (lap_count went up).
__device__ __forceinline__ bool lmpc_fleet_record_car(const lmpc_fleet_store& st, int b, const double* x, double u0, double u1, double k,
                                                      double t, double Lt) {
  const double s = x[0];
  int fl = st.flags[b];
  if (!(fl & LMPC_FLEET_FLAG_VALID)) {  // the very first sample only seeds the abscissa (:278-282)
    st.s_prev[b] = s;
    st.flags[b] = fl | LMPC_FLEET_FLAG_VALID;
    return false;
  }
  const double sp = st.s_prev[b];
  st.s_prev[b] = s;
  const int R1 = st.R + 1, C = st.C;
  int head = st.head[b], at = -1;
  bool crossed = false;
  if (sp - s > 0.5 * Lt) {  // crossed the start line
    crossed = true;
    if (fl & LMPC_FLEET_FLAG_INIT) {
      const size_t slot = (size_t)b * R1 + head;
      const int dn = st.dur_n[b];
      st.dur[(size_t)b * LMPC_FLEET_DUR + dn % LMPC_FLEET_DUR] = t - st.aux[slot * C * 4 + 3];  // t at the crossing - t of the lap's first sample
      st.dur_n[b] = dn + 1;
      if (fl & LMPC_FLEET_FLAG_OVERFLOW) {  // longer than a slot: not added, nothing evicted; the slot is reused for the next lap
        st.n_dropped[b] += 1;
      } else {  // the open lap becomes the newest of the ring where it stands; the next slot (unused, or the oldest lap) opens
        st.npts[slot] = st.open_n[b];
        head = head + 1 == R1 ? 0 : head + 1;
        st.head[b] = head;
        const int c = st.cnt[b];
        if (c < st.R) st.cnt[b] = c + 1;
      }
    }  // else: the first, partial lap is discarded (:296-300)
    st.flags[b] = (fl | LMPC_FLEET_FLAG_INIT) & ~LMPC_FLEET_FLAG_OVERFLOW;
    st.lap_count[b] += 1;
    st.open_n[b] = 1;  // the closing sample starts the next lap
    at = 0;
  } else if (fl & LMPC_FLEET_FLAG_INIT) {
    const int n = st.open_n[b];
    if (n < C) {
      at = n;
      st.open_n[b] = n + 1;
    } else if (!(fl & LMPC_FLEET_FLAG_OVERFLOW)) {  // the slot is full: the lap stops storing and will be dropped at its close
      st.flags[b] = fl | LMPC_FLEET_FLAG_OVERFLOW;
    }
  }
  if (at < 0) return crossed;
  const size_t row = ((size_t)b * R1 + head) * C + at;  // at < C, head <= R: inside car b's slots
  st.key[row] = make_double2(s, x[1]);
  double* xr = st.xr + row * 4;
  double* ax = st.aux + row * 4;
#pragma unroll
  for (int c = 0; c < 4; ++c) xr[c] = x[2 + c];
  ax[0] = u0;
  ax[1] = u1;
  ax[2] = k;
  ax[3] = t;
  return crossed;
}

#endif  // LMPC_LOOP_STEPS_HIP_H_
