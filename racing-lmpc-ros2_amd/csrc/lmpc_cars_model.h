// lmpc_cars_model.h -- the per-car single-track CONTROLLER model of include/lmpc_hip_cars_model.h: the launcher of
// lmpc_linearize_cars_kernel (csrc/lmpc_cars_model_kernel.hip), as the host layer calls it (lmpc_linearize_cars_batch, and solve_batch /
// lmpc_solve_batch_f32 while lmpc_cars_set_controller_model is on, in csrc/lmpc_capi.hip).  The table it reads is csrc/lmpc_cars.h's.
#ifndef LMPC_CARS_MODEL_H_
#define LMPC_CARS_MODEL_H_

#include <hip/hip_runtime.h>

#include "lmpc_cars.h"

// Defined in lmpc_cars_model_kernel.hip, a translation unit of its own (adding it leaves the device code of the other units as it
// was).  One launch on `stream`: tab is a car table of B vehicles, problem b of N knots linearised on vehicle b about X_ref [6][N][B],
// U_ref [2][N-1][B] with T_ref [N-1][B] and curv [N][B].  ws: A is the linearisation workspace [B][N-1][LMPC_LIN_RECORD] (Bm, g
// unused); otherwise the A / Bm / g arrays of lmpc_linearize_batch.  io = double, or float for the single-precision solve (ws only).
__attribute__((visibility("hidden"))) hipError_t lmpc_cars_launch_linearize(hipStream_t stream, const double* tab, int N, int B, bool ws,
                                                                            const double* X_ref, const double* U_ref, const double* T_ref,
                                                                            const double* curv, double* A, double* Bm, double* g);
__attribute__((visibility("hidden"))) hipError_t lmpc_cars_launch_linearize_f32(hipStream_t stream, const double* tab, int N, int B,
                                                                                const float* X_ref, const float* U_ref, const float* T_ref,
                                                                                const float* curv, float* ws);

#endif  // LMPC_CARS_MODEL_H_
