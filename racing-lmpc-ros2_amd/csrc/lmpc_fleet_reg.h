// lmpc_fleet_reg.h -- the per-car error-dynamics regression on the fleet safe set (csrc/lmpc_fleet_reg_kernel.hip; entry points
// lmpc_fleet_ss_set_regression / lmpc_fleet_ss_regress_batch in csrc/lmpc_capi.hip).
//
// Per car one dense table of the samples of its closed laps that have a successor, laps oldest first, samples in order:
//   tab [car][cap][NF + NOUT + 1]   z (NF features) | y (NOUT one-step residuals of the nominal model) | |z|^2
//   nrow [car]                      rows in use, padded to a multiple of four with rows no query can reach (z = 0, |z|^2 = 1e30)
//   stamp [car]                     the car's lap_count when its table was packed; LMPC_FLEET_REG_STALE = pack again
// cap = max_lap_stored x (max_pts_per_lap - 1) rounded up to four: a ring cannot hold more samples with a successor.
// (5, 3): 72 bytes per row, (8, 6): 120.  lmpc_fleet_ss_set_regression allocates all three; nothing later allocates.
#ifndef LMPC_FLEET_REG_H_
#define LMPC_FLEET_REG_H_

#include <hip/hip_runtime.h>

#include "lmpc_device.h"
#include "lmpc_fleet_ss.h"
#include "lmpc_reg_rows.h"

#define LMPC_FLEET_REG_STALE (-1)  // no lap_count is negative; a memset of 0xff bytes writes it

struct lmpc_fleet_reg_table {
  int cap = 0;  // rows per car
  double* tab = nullptr;
  int* nrow = nullptr;
  int* stamp = nullptr;
};

static inline int lmpc_fleet_reg_cap(int R, int C) { return (int)(((long long)R * (C - 1) + 3) / 4 * 4); }

// The two launches of one regression, on `stream`: the pack kernel (a car whose stamp equals its lap_count returns at once) and
// lmpc_fleet_regress_kernel<NF, NOUT, ws> for spec's (5, 3) or (8, 6).  ws: A is the linearisation workspace [B][N-1][54] and Bm, g
// are unused; otherwise the arrays of lmpc_linearize_batch.  Defined in lmpc_fleet_reg_kernel.hip, a translation unit of its own.
__attribute__((visibility("hidden"))) hipError_t lmpc_fleet_reg_launch(hipStream_t stream, const lmpc_fleet_store& st, const lmpc_vehicle& veh,
                                                                       const lmpc_regression_spec& spec, const lmpc_fleet_reg_table& tb, int N,
                                                                       bool ws, const double* X_ref, const double* U_ref, double* A, double* Bm,
                                                                       double* g);

// The same two launches for a per-row spec (lmpc_fleet_ss_set_regression_rows; csrc/lmpc_fleet_reg_rows_kernel.hip): the table's row is
// lmpc_reg_rows.h's, 3 MF + 3 doubles -- 120 bytes for MF = 4, 144 for MF = 5 -- in the same three allocations.
__attribute__((visibility("hidden"))) hipError_t lmpc_fleet_reg_rows_launch(hipStream_t stream, const lmpc_fleet_store& st, const lmpc_vehicle& veh,
                                                                            const lmpc_reg_rows_dev& spec, const lmpc_fleet_reg_table& tb, int N,
                                                                            bool ws, const double* X_ref, const double* U_ref, double* A,
                                                                            double* Bm, double* g);

#endif  // LMPC_FLEET_REG_H_
