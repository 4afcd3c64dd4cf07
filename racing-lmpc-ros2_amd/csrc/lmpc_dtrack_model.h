// lmpc_dtrack_model.h -- the double-track CONTROLLER model of include/lmpc_hip_dtrack_model.h: the launcher of
// lmpc_linearize_dtrack_kernel (csrc/lmpc_dtrack_model_kernel.hip), as the host layer calls it (lmpc_linearize_dtrack_batch, and
// solve_batch while lmpc_dtrack_set_controller_model is on, in csrc/lmpc_capi.hip).  The table it reads is csrc/lmpc_dtrack.h's.
#ifndef LMPC_DTRACK_MODEL_H_
#define LMPC_DTRACK_MODEL_H_

#include <hip/hip_runtime.h>

#include "lmpc_dtrack.h"

// Defined in lmpc_dtrack_model_kernel.hip, a translation unit of its own (adding it leaves the device code of the other units as it
// was).  One launch on `stream`: tab is a table of B vehicles, problem b of N knots linearised on vehicle b about X_ref [6][N][B],
// U_ref [2][N-1][B] with T_ref [N-1][B] and curv [N][B].  ws: A is the linearisation workspace [B][N-1][LMPC_LIN_RECORD] (Bm, g
// unused); otherwise the A / Bm / g arrays of lmpc_linearize_batch.
__attribute__((visibility("hidden"))) hipError_t lmpc_dtrack_launch_linearize(hipStream_t stream, const double* tab, int N, int B, bool ws,
                                                                              const double* X_ref, const double* U_ref, const double* T_ref,
                                                                              const double* curv, double* A, double* Bm, double* g);

#endif  // LMPC_DTRACK_MODEL_H_
