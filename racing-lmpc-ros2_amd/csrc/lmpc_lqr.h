// lmpc_lqr.h -- the batched time-varying LQR, one controller per car (csrc/lmpc_lqr_kernel.hip; entry points lmpc_lqr_* in
// csrc/lmpc_capi.hip).  Restates RacingLQR::solve (racing_lqr.cpp:45-96) over the single-track model with k = 0: per stage the
// continuous Jacobian at the reference point, its exact zero-order-hold discretisation expm([[Ac, Bc], [0, 0]] dt)
// (lmpc_utils/src/utils.cpp:52-65), one backward Riccati recursion with general (never symmetrised) Q, R, Qf, and one closed-loop
// rollout that is always RK4, whatever the vehicle's integrator.
//
// Handle-owned workspace (lmpc_lqr_create), laid out for the batch of the call (batch <= max_batch), eight lanes per problem:
//   cfg [76]                 Q [36] | R [4] | Qf [36], row-major
//   AB  [N-1][8][B][6]       column c of [A_k | B_k] of car b, its six rows side by side: the six row lanes of the eight cars of a
//                            wave write 48 consecutive doubles per column
//   K   [N-1][2][B][6]       row i of K_k of car b; lane c writes column c and is the only lane that reads it back
// A solve is two launches: lmpc_lqr_discretize_kernel over (car, stage) and lmpc_lqr_recursion_kernel over cars.
#ifndef LMPC_LQR_H_
#define LMPC_LQR_H_

#include <hip/hip_runtime.h>

#include "lmpc_device.h"

#define LMPC_LQR_NOT_FINITE 1  // flags bit 0: the car's X_optm, U_optm, K or P0 holds a NaN or Inf

// expm: [[Ac, Bc], [0, 0]] dt is halved until its infinity norm is <= 1/2 (at most LMPC_LQR_SQUARINGS_MAX times; a norm that is
// still larger then, or not finite, poisons the stage with NaN and the car ends flagged), a Taylor polynomial of degree
// LMPC_LQR_TAYLOR_DEGREE (remainder 0.5^15 / 15! = 2e-17), and as many squarings as halvings.
#define LMPC_LQR_SQUARINGS_MAX 20
#define LMPC_LQR_TAYLOR_DEGREE 14

struct lmpc_lqr_store {
  int max_batch = 0;  // 0: no controller
  int N = 0;
  double dt = 0.0;
  double* cfg = nullptr;
  double* AB = nullptr;
  double* K = nullptr;
};

struct lmpc_lqr_io {  // the caller's arrays, batch fastest
  const double* x_ic;   // [6][B]
  const double* X_ref;  // [6][N][B]
  const double* U_ref;  // [2][N-1][B]
  double* X_optm;       // [6][N][B]
  double* U_optm;       // [2][N-1][B]
  double* K;            // [2][6][N-1][B] or null
  double* P0;           // [36][B] or null
  int* flags;           // [B] or null
};

// One solve of `batch` cars on `stream`.  Defined in lmpc_lqr_kernel.hip, a translation unit of its own.
__attribute__((visibility("hidden"))) hipError_t lmpc_lqr_launch(hipStream_t stream, const lmpc_lqr_store& st, const lmpc_vehicle& veh, int batch,
                                                                 const lmpc_lqr_io& io);

#endif  // LMPC_LQR_H_
