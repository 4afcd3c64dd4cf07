// lmpc_reg_rows.h -- the error-dynamics regression with one feature list per regressed row (lmpc_regression_rows_spec,
// include/lmpc_hip.h): what the host layer hands the kernels of lmpc_reg_rows_kernel.hip (one shared table) and
// lmpc_fleet_reg_rows_kernel.hip (one table per car), and the one place the spec is validated.
//
// A sample's row of either table, for the instance with MF features per regressed row (MF = 4 or 5), always three rows:
//   [ z_0 (MF) | z_1 (MF) | z_2 (MF) | y_0 y_1 y_2 ]      3 MF + 3 doubles: 120 bytes for MF = 4, 144 for MF = 5
// z_o = [x[S_o]; u[C_o]] of row o's own lists, zero behind its last feature; y_o the nominal model's one-step residual of state out[o].
// A null feature is 0 in the table and in the query: its row and column of M'KM + 1e-3 I are 1e-3 on the diagonal and 0 elsewhere,
// it sits between the real features and the constant, decouples exactly (every product it enters is with an exact 0) and nothing is
// scattered for it.  A row the spec does not use (n_out < 3) is all null, and the query's first feature of it is 1e30: no sample is
// within its bandwidth.  A padding sample (tables are padded to a multiple of four) has 1e15 in the first feature of every row.
#ifndef LMPC_REG_ROWS_H_
#define LMPC_REG_ROWS_H_

#include "lmpc_hip.h"

#define LMPC_REG_ROWS 3       // regressed rows of an instance
#define LMPC_REG_ROWS_MAXF 5  // features per row, at most
#define LMPC_REG_ROWS_STRIDE(MF) (LMPC_REG_ROWS * (MF) + LMPC_REG_ROWS)
#define LMPC_REG_ROWS_FAR_Z 1e15  // first feature of a padding sample
#define LMPC_REG_ROWS_FAR_Q 1e30  // first feature of a query that takes no sample (a dead lane, an unused row)

// The spec as the kernels read it.  Passed by value as a kernel argument.
struct lmpc_reg_rows_dev {
  int n_out;                                     // rows in use, 1 .. 3
  int mf;                                        // the instance: 4 or 5 features per row (the longest list decides)
  int out[LMPC_REG_ROWS];                        // regressed state per row
  int nf[LMPC_REG_ROWS];                         // features of row o; 0 for a row not in use
  int col[LMPC_REG_ROWS][LMPC_REG_ROWS_MAXF];    // feature f of row o as a column of [A B]: a state index, or 6 + a control index
  int as_written;
  double dist_max;
};

static inline int lmpc_reg_rows_stride(const lmpc_reg_rows_dev& d) { return LMPC_REG_ROWS_STRIDE(d.mf); }

// Validates `spec` and digests it into `d`.  LMPC_OK, or the error code with *msg set; `d` is written only on LMPC_OK.
static inline int lmpc_reg_rows_digest(const lmpc_regression_rows_spec* spec, lmpc_reg_rows_dev* d, const char** msg) {
  static const char* const limits =
      "per-row regression built for 1 .. 3 rows of 1 .. 5 features each (n_in_state + n_in_ctrl), at least one of them a state";
  if (spec->n_out < 1 || spec->n_out > LMPC_REG_ROWS) return *msg = limits, LMPC_ERR_UNSUPPORTED;
  for (int o = 0; o < spec->n_out; ++o) {
    const int ns = spec->n_in_state[o], nc = spec->n_in_ctrl[o];
    if (ns < 1 || ns > 6 || nc < 0 || nc > 2 || ns + nc > LMPC_REG_ROWS_MAXF) return *msg = limits, LMPC_ERR_UNSUPPORTED;
  }
  if (!(spec->dist_max > 0.0)) return *msg = "dist_max must be positive", LMPC_ERR_ARGUMENT;
  lmpc_reg_rows_dev r{};
  r.n_out = spec->n_out;
  r.mf = 4;
  r.as_written = spec->as_written ? 1 : 0;
  r.dist_max = spec->dist_max;
  for (int o = 0; o < spec->n_out; ++o) {
    const int ns = spec->n_in_state[o], nc = spec->n_in_ctrl[o];
    if (spec->out[o] < 0 || spec->out[o] > 5) return *msg = "regressed row out of range", LMPC_ERR_ARGUMENT;
    for (int p = 0; p < o; ++p)
      if (spec->out[p] == spec->out[o]) return *msg = "a state is regressed by one row only", LMPC_ERR_ARGUMENT;
    for (int f = 0; f < ns; ++f) {
      if (spec->in_state[o][f] < 0 || spec->in_state[o][f] > 5) return *msg = "feature state out of range", LMPC_ERR_ARGUMENT;
      for (int p = 0; p < f; ++p)
        if (spec->in_state[o][p] == spec->in_state[o][f]) return *msg = "a feature state is listed twice in one row", LMPC_ERR_ARGUMENT;
      r.col[o][f] = spec->in_state[o][f];
    }
    for (int f = 0; f < nc; ++f) {
      if (spec->in_ctrl[o][f] < 0 || spec->in_ctrl[o][f] > 1) return *msg = "feature control out of range", LMPC_ERR_ARGUMENT;
      for (int p = 0; p < f; ++p)
        if (spec->in_ctrl[o][p] == spec->in_ctrl[o][f]) return *msg = "a feature control is listed twice in one row", LMPC_ERR_ARGUMENT;
      r.col[o][ns + f] = 6 + spec->in_ctrl[o][f];
    }
    r.out[o] = spec->out[o];
    r.nf[o] = ns + nc;
    if (ns + nc > r.mf) r.mf = ns + nc;
  }
  *d = r;
  return LMPC_OK;
}

#endif  // LMPC_REG_ROWS_H_
