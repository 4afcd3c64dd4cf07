/*
 * lmpc_hip_rows.h -- the error-dynamics regression with ONE FEATURE LIST PER REGRESSED ROW: its spec and its two entry points.
 * Part of the C ABI of lmpc_hip.h, which includes this file (include lmpc_hip.h, not this file alone); every convention of that
 * header holds here -- return codes, device pointers, the stream rule.  The stream class of the two entry points: both are
 * BLOCKING, lmpc_set_regression_laps_rows moves its host arrays with the synchronous hipMemcpy between waits on the handle's stream
 * as lmpc_set_regression_laps does.  tests/test_stream_table_rows.py holds one class per prototype of this file and
 * tests/test_gpu_streams_rows.py holds both to it on a stream that is held by a timed gate.
 */
#ifndef LMPC_HIP_ROWS_H_
#define LMPC_HIP_ROWS_H_

#ifndef LMPC_HIP_H_
#error "include lmpc_hip.h: it includes lmpc_hip_rows.h"
#endif

/* The regression of lmpc_set_regression_laps with ONE FEATURE LIST PER REGRESSED ROW, as RegQuery carries them (reg_in_state_idxs,
 * reg_in_control_idxs and reg_out_state_idxs are vectors of vectors, safe_set.hpp:61-75): the longitudinal row on the speeds and
 * the longitudinal input, the lateral and yaw rows on the speeds and the steering angle.  For row o with r = out[o],
 * S_o = in_state[o][:n_in_state[o]] and C_o = in_ctrl[o][:n_in_ctrl[o]]:
 *   z_j = [x_j[S_o]; u_j[C_o]],  q = [X_ref[S_o]; U_ref[C_o]],  d_j = ||z_j - q||_2 in that row's own feature space,
 *   candidates d_j < dist_max, K_j, M = [z_j' 1], Q = M'KM + 1e-3 I and the sign switch as at lmpc_set_regression_laps,
 *   R = Q^-1 (+-M'K y_r),  A[r, S_o] += R[0:ns_o],  B[r, C_o] += R[ns_o:-1],  g[r] += R[-1].
 * The residuals y_r are the nominal model's on the full recorded state, as there; the weights are always formed from
 * sum (z - q)^2.  A row without a candidate leaves its entries bit-identical while other rows of the same query are corrected.
 * It is the one-list regression of row r on (S_o, C_o), row after row (oracle/regression.py with out_rows = (r,)), in ONE pass over
 * the samples for all rows.
 * Built for n_out = 1 .. 3 and per row 1 <= n_in_state + n_in_ctrl <= 5 with n_in_state >= 1; the lengths may differ between
 * rows.  Other sizes: LMPC_ERR_UNSUPPORTED.  An index out of range, a duplicate within a list or in out, dist_max <= 0:
 * LMPC_ERR_ARGUMENT. */
typedef struct lmpc_regression_rows_spec {
  int32_t n_out;            /* regressed rows, 1 .. 3 */
  int32_t out[6];           /* one state index per row, no duplicates */
  int32_t n_in_state[6];    /* per row */
  int32_t in_state[6][6];
  int32_t n_in_ctrl[6];     /* per row */
  int32_t in_ctrl[6][2];
  int32_t as_written;       /* as in lmpc_regression_spec */
  double  dist_max;         /* one bandwidth for all rows, as RegQuery has one */
} lmpc_regression_rows_spec;

/* lmpc_set_regression_laps with a per-row spec: same HOST arrays, same store (either form replaces the other: a handle holds one
 * shared regression), same rules -- n_laps = 0 or spec = NULL switches the regression off; with laps it is refused
 * (LMPC_ERR_ARGUMENT) while a per-car regression of either form is in effect; while it is on, lmpc_regress_batch and every fp64 /
 * mixed batched solve apply it where they apply the one-list form, and lmpc_solve_batch_f32 returns LMPC_ERR_UNSUPPORTED.  A refused
 * call changes nothing: the regression in effect before it stays.  Blocking: it synchronises the handle's stream before the old
 * tables are freed and again behind the kernels that build the new ones, and moves its host arrays with synchronous copies. */
int lmpc_set_regression_laps_rows(lmpc_handle* h, int32_t n_laps, const int32_t* n_pts, const double* x, const double* u,
                                  const double* k, const double* t, const lmpc_regression_rows_spec* spec);

/* lmpc_fleet_ss_set_regression with one feature list per regressed row: query (b, i) regresses every row of the spec, each in its
 * own feature space, on the closed laps in car b's ring.  Everything
 * else is lmpc_fleet_ss_set_regression's: it uploads no data, needs a fleet store, validates the spec as
 * lmpc_set_regression_laps_rows does, is refused (LMPC_ERR_ARGUMENT) while a shared regression of either form is in effect, and a
 * refused call changes nothing.  Either form replaces the other on the store.  Per car it allocates max_lap_stored x
 * (max_pts_per_lap - 1) samples rounded up to four of 8 (3 MF + 3) bytes each, MF = 4 or 5 by the longest list of the spec -- 120 or
 * 144 bytes; lmpc_fleet_ss_bytes includes it -- and nothing later allocates.  A new spec or sign sets every car's stamp stale (every
 * table is filled again in front of the next use).  It synchronises the handle's stream only when the table's size changes.  Otherwise
 * it enqueues two memsets on it and returns.  spec = NULL switches the per-car regression off (either form).
 * While it is on, lmpc_fleet_ss_regress_batch and every solve that applies the one-list per-car regression apply this one, under
 * the same batch rule; lmpc_solve_batch_f32 returns LMPC_ERR_UNSUPPORTED. */
int lmpc_fleet_ss_set_regression_rows(lmpc_handle* h, const lmpc_regression_rows_spec* spec);

#endif  /* LMPC_HIP_ROWS_H_ */
