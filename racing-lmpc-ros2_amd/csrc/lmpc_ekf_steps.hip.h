// lmpc_ekf_steps.hip.h -- what one car's filter does in an update of the batched extended Kalman filter (csrc/lmpc_ekf.h), as the
// kernels that run it share it: the prediction and the correction by an observation of NZ rows.  One text for each step:
// lmpc_ekf_predict_kernel and lmpc_ekf_correct_kernel<NZ> (lmpc_ekf_kernel.hip) are thin wrappers over these functions, and
// lmpc_estimated_loop_kernel (lmpc_estimated_loop_kernel.hip) chains them with the plant, the sensors and the projection.
//   lmpc_ekf_predict_car      x_p = f_d(x, u, k = 0, dt), P_p = F P F' + Q   (ekf_state_estimator.cpp:142-146)
//   lmpc_ekf_correct_car<NZ>  y, S, K, x, P, the NaN / Inf fallback, check_cov, the clip   (:155-202, :238-264)
// F is never formed.  The four RK4 points' sparse partials are kept (lmpc_fjac J[4]) and a vector is pushed through the stage chain
// with lmpc_jvp, as lmpc_linearize_kernel pushes its unit vectors: first the six columns of P (M = F P, written over P), then the six
// rows of M (row j of F M' is row j of P_p = M F', written over row j of M).  One vector at a time (`unroll 1`): the loop shape that
// keeps the linearisation kernel's live set small.
// Both work on car b of the store in place, in global memory: a thread reads back only what it wrote itself.
#ifndef LMPC_EKF_STEPS_HIP_H_
#define LMPC_EKF_STEPS_HIP_H_

#include <hip/hip_runtime.h>

#include "lmpc_device.h"
#include "lmpc_dynamics.hip.h"
#include "lmpc_ekf.h"

// lmpc::utils::align_yaw (lmpc_utils/utils.hpp:25-31), the expression track_align_yaw of lmpc_track.hip.h evaluates
__device__ __forceinline__ double ekf_align_yaw(double yaw_1, double yaw_2) {
#pragma clang fp contract(off)
  const double d = yaw_1 - yaw_2;
  return atan2(sin(d), cos(d)) + yaw_2;
}

// std::clamp (ekf_state_estimator.cpp:199-202): a NaN passes through
__device__ __forceinline__ double ekf_clamp(double v, double lo, double hi) { return v < lo ? lo : (hi < v ? hi : v); }

__device__ __forceinline__ bool ekf_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }

// The prediction of car b over dt.  `final`: the update has no observation -- clip and write the caller's arrays here; the value
// returned is then whether the new estimate and covariance are finite (else true).  Otherwise x_p goes to the store unclipped and
// lmpc_ekf_correct_car finishes the update.
__device__ __forceinline__ bool lmpc_ekf_predict_car(const lmpc_vehicle& veh, const lmpc_ekf_consts& cst, const lmpc_ekf_store& st, int b, double dt,
                                                     int final, const lmpc_ekf_out& out) {
  const size_t B = (size_t)st.B;
  double x[6], u[2];
#pragma unroll
  for (int k = 0; k < 6; ++k) x[k] = st.x[k * B + b];
#pragma unroll
  for (int k = 0; k < 2; ++k) u[k] = st.u[k * B + b];

  lmpc_uterms ut;
  lmpc_u_terms(veh, u[0], u[1], ut);
  lmpc_fjac J[4];
  double ks[4][6], xs[6];
  const double cs[4] = {0.0, 0.5, 0.5, 1.0};
#pragma unroll
  for (int s = 0; s < 4; ++s) {
#pragma unroll
    for (int r = 0; r < 6; ++r) xs[r] = (s == 0) ? x[r] : x[r] + cs[s] * dt * ks[s - 1][r];
    lmpc_f<true>(veh, ut, xs, 0.0, ks[s], &J[s]);
  }
  // the four slopes' weights: dt/6 (1, 2, 2, 1), or the first slope alone (Euler, utils.cpp:110-123), as in lmpc_linearize_kernel
  const bool euler = veh.integrator == LMPC_INTEGRATOR_EULER;
  const double wgt[4] = {euler ? dt : dt / 6, euler ? 0.0 : dt / 3, euler ? 0.0 : dt / 3, euler ? 0.0 : dt / 6};
  bool ok = true;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    double xp = x[r] + (wgt[0] * ks[0][r] + wgt[1] * ks[1][r] + wgt[2] * ks[2][r] + wgt[3] * ks[3][r]);
    if (final) {
      xp = ekf_clamp(xp, cst.x_min[r], cst.x_max[r]);
      ok = ok && ekf_finite(xp);
      if (out.x) out.x[r * B + b] = xp;
    }
    st.x[r * B + b] = xp;
  }
  const double tu[2] = {0.0, 0.0};
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
#pragma unroll 1
    for (int c = 0; c < 6; ++c) {
      // pass 0: column c of P (stride 6 between its rows); pass 1: row c of M = F P (contiguous)
      const size_t first = pass ? (size_t)c * 6 : (size_t)c, step = pass ? 1 : 6;
      double e[6], tx[6], kc[6], acc[6];
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        e[r] = st.P[(first + r * step) * B + b];
        tx[r] = e[r];
        acc[r] = 0.0;
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        lmpc_jvp(J[s], tx, tu, kc);
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          acc[r] += wgt[s] * kc[r];
          if (s < 3) tx[r] = e[r] + cs[s + 1] * dt * kc[r];
        }
      }
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        double d = e[r] + acc[r];
        if (pass) {
          d += cst.Q[c * 6 + r];  // Q once per update, whatever dt is (:146)
          if (final) {
            ok = ok && ekf_finite(d);
            if (out.P) out.P[(first + r * step) * B + b] = d;
          }
        }
        st.P[(first + r * step) * B + b] = d;
      }
    }
  }
  return ok;
}

// The correction of car b by an observation of NZ selected rows, zv [NZ] the car's measurement (in registers), R [NZ][NZ][B].  S' K' =
// (P_p H')' is solved in registers by Gaussian elimination with row pivoting, fully unrolled (the row exchanges are selects); nothing
// is indexed at run time but global memory, where the observation's rows address P_p and x_p directly.  xe [6] out: the new estimate,
// as it went to the store.  Returns the car's flags (LMPC_EKF_*).
template <int NZ>
__device__ __forceinline__ int lmpc_ekf_correct_car(const lmpc_ekf_consts& cst, const lmpc_ekf_store& st, const lmpc_ekf_obs& ob, int b, const double* zv,
                                                    const double* __restrict__ R, const lmpc_ekf_out& out, double* xe) {
  const size_t B = (size_t)st.B;
  double Rv[NZ][NZ];
  bool bad = false;
#pragma unroll
  for (int a = 0; a < NZ; ++a) {
    bad = bad || !ekf_finite(zv[a]);
#pragma unroll
    for (int c = 0; c < NZ; ++c) {
      Rv[a][c] = R[(size_t)(a * NZ + c) * B + b];
      bad = bad || !ekf_finite(Rv[a][c]);
    }
  }
  int flags = bad ? LMPC_EKF_FALLBACK : 0;
  double xn[6];
#pragma unroll
  for (int r = 0; r < 6; ++r) xn[r] = st.x[r * B + b];  // x_p
  bool ok = true;
  if (!bad) {
    // check_cov as written (:244-255): the inner loop advances i, so only column 0 is visited
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
      if (Rv[i][0] < 0.0) Rv[i][0] = 0.0, flags |= LMPC_EKF_R_REPAIRED;
      if (i == 0 && Rv[0][0] <= 0.0) Rv[0][0] = 1e-6, flags |= LMPC_EKF_R_REPAIRED;
    }
    // A = [S' | (P_p H')'],  S = H P_p H' + R,  (P_p H')[i][a] = P_p[i][rows[a]];  HP[a][j] = P_p[rows[a]][j]
    double A[NZ][NZ + 6], HP[NZ][6], y[NZ];
#pragma unroll
    for (int a = 0; a < NZ; ++a) {
#pragma unroll
      for (int c = 0; c < NZ; ++c) A[a][c] = st.P[(size_t)(ob.rows[c] * 6 + ob.rows[a]) * B + b] + Rv[c][a];
#pragma unroll
      for (int i = 0; i < 6; ++i) A[a][NZ + i] = st.P[(size_t)(i * 6 + ob.rows[a]) * B + b];
#pragma unroll
      for (int j = 0; j < 6; ++j) HP[a][j] = st.P[(size_t)(ob.rows[a] * 6 + j) * B + b];
      double hx = st.x[(size_t)ob.rows[a] * B + b];
      if (ob.rows[a] == 2) hx = ekf_align_yaw(hx, zv[a]);  // h's second argument upstream: the yaw is aligned to the measurement
      y[a] = zv[a] - hx;
    }
#pragma unroll
    for (int k = 0; k < NZ; ++k) {
#pragma unroll
      for (int i = k + 1; i < NZ; ++i) {  // after this loop row k holds the largest |A[.][k]| of rows k ..
        const bool sw = fabs(A[i][k]) > fabs(A[k][k]);
#pragma unroll
        for (int c = k; c < NZ + 6; ++c) {
          const double lo = A[k][c], hi = A[i][c];
          A[k][c] = sw ? hi : lo;
          A[i][c] = sw ? lo : hi;
        }
      }
#pragma unroll
      for (int i = k + 1; i < NZ; ++i) {
        const double f = A[i][k] / A[k][k];
#pragma unroll
        for (int c = k + 1; c < NZ + 6; ++c) A[i][c] -= f * A[k][c];
      }
    }
#pragma unroll
    for (int k = NZ - 1; k >= 0; --k) {  // back substitution: A[k][NZ + i] becomes K[i][k]
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        double v = A[k][NZ + i];
#pragma unroll
        for (int c = k + 1; c < NZ; ++c) v -= A[k][c] * A[c][NZ + i];
        A[k][NZ + i] = v / A[k][k];
      }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double dx = 0.0;
#pragma unroll
      for (int a = 0; a < NZ; ++a) {
        const double kia = A[a][NZ + i];
        dx += kia * y[a];
        st.K[((size_t)i * st.nzsum + ob.koff + a) * B + b] = kia;
        if (out.Kz) out.Kz[(size_t)(i * NZ + a) * B + b] = kia;
      }
      xn[i] += dx;
#pragma unroll
      for (int j = 0; j < 6; ++j) {  // P = (I - K H) P_p = P_p - K (H P_p), entry by entry, in place
        double p = st.P[(size_t)(i * 6 + j) * B + b];
#pragma unroll
        for (int a = 0; a < NZ; ++a) p -= A[a][NZ + i] * HP[a][j];
        st.P[(size_t)(i * 6 + j) * B + b] = p;
        ok = ok && ekf_finite(p);
        if (out.P) out.P[(size_t)(i * 6 + j) * B + b] = p;
      }
    }
  } else {
    // pure prediction for this car: P_p stays, its slice of K stays (and is what Kz reports, :208)
#pragma unroll 1
    for (int e = 0; e < 36; ++e) {
      const double p = st.P[(size_t)e * B + b];
      ok = ok && ekf_finite(p);
      if (out.P) out.P[(size_t)e * B + b] = p;
    }
    if (out.Kz) {
#pragma unroll 1
      for (int i = 0; i < 6; ++i)
        for (int a = 0; a < NZ; ++a) out.Kz[(size_t)(i * NZ + a) * B + b] = st.K[((size_t)i * st.nzsum + ob.koff + a) * B + b];
    }
  }
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const double v = ekf_clamp(xn[r], cst.x_min[r], cst.x_max[r]);
    ok = ok && ekf_finite(v);
    st.x[r * B + b] = v;
    if (out.x) out.x[r * B + b] = v;
    xe[r] = v;
  }
  return flags | (ok ? 0 : LMPC_EKF_NOT_FINITE);
}

#endif  // LMPC_EKF_STEPS_HIP_H_
