// lmpc_ekf.h -- the batched extended Kalman filter, one filter per car (csrc/lmpc_ekf_kernel.hip; entry points lmpc_ekf_* in
// csrc/lmpc_capi.hip).  Restates EKFStateEstimator::update_observation (ekf_state_estimator.cpp:112-214) over the single-track
// model with k = 0, where the Frenet rows (s, e_y, e_psi) are the global ones (X, Y, yaw).
//
// Handle-owned store, struct of arrays with the batch axis fastest (every access of a wave is one coalesced transaction):
//   x [6][B]          the estimate           u [2][B]   the control held over a prediction (update_control)
//   P [36][B]         the covariance, row-major, all 36 entries (the correction is the non-symmetric (I - K H) P_p, as written)
//   K [6][nzsum][B]   the gain of every registered observation side by side; an update overwrites its own columns only
// An update is two launches: lmpc_ekf_predict_kernel (x_p into x, P_p = F P F' + Q into P, in place) and, with an observation,
// lmpc_ekf_correct_kernel<nz> (innovation, gain, correction, clip -- or, for a car whose z or R is not finite, the clip alone).
#ifndef LMPC_EKF_H_
#define LMPC_EKF_H_

#include <hip/hip_runtime.h>

#include "lmpc_device.h"

#define LMPC_EKF_FALLBACK 1   // flags bit 0: NaN / Inf in z or R, the car took the pure prediction (:158-167)
#define LMPC_EKF_R_REPAIRED 2 // flags bit 1: check_cov changed the kernel's copy of R (:238-264)
#define LMPC_EKF_NOT_FINITE 4 // flags bit 2: the new estimate or covariance holds a NaN or Inf

struct lmpc_ekf_store {
  int B = 0;      // cars
  int nzsum = 0;  // columns of K
  double* x = nullptr;
  double* u = nullptr;
  double* P = nullptr;
  double* K = nullptr;
};

struct lmpc_ekf_consts {  // by value in the kernel arguments
  double Q[36];
  double x_min[6], x_max[6];
};

struct lmpc_ekf_obs {
  int nz;       // 1 .. 6
  int koff;     // first column of its slice of K
  int rows[6];  // the state rows h selects, in the order of z
};

struct lmpc_ekf_out {  // the caller's arrays, any of them null
  double* x;   // [6][B]
  double* P;   // [36][B]
  double* Kz;  // [6][nz][B]
  int* flags;  // [B]
};

// One update on `stream`: the prediction over dt and, with obs != null, the correction by z [nz][B], R [nz][nz][B].
// Defined in lmpc_ekf_kernel.hip, a translation unit of its own.
__attribute__((visibility("hidden"))) hipError_t lmpc_ekf_launch(hipStream_t stream, const lmpc_ekf_store& st, const lmpc_vehicle& veh,
                                                                 const lmpc_ekf_consts& cst, const lmpc_ekf_obs* obs, double dt,
                                                                 const double* z, const double* R, const lmpc_ekf_out& out);

struct lmpc_ekf_seed {  // the config's start, by value in the kernel arguments
  double x0[6], P0[36];
};

// x [6][B] <- xs (null: x0 for every car), P [36][B] <- Ps (null: P0)
__attribute__((visibility("hidden"))) hipError_t lmpc_ekf_seed_launch(hipStream_t stream, const lmpc_ekf_store& st, const lmpc_ekf_seed& seed,
                                                                      const double* xs, const double* Ps);

#endif  // LMPC_EKF_H_
