// lmpc_reg_rows_core.hip.h -- the per-row error-dynamics regression, once: what lmpc_regress_rows_kernel (lmpc_reg_rows_kernel.hip:
// one lane per query of any car, one shared table) and lmpc_fleet_regress_rows_kernel (lmpc_fleet_reg_rows_kernel.hip: one wavefront
// per car, the car's own table) both do for a lane's query, and what the kernels that build their tables both do for a sample.
// The kernels keep how a lane gets its (b, i, live) and where a group of rows comes from.  Table layout: lmpc_reg_rows.h.
//
//   per sample   lmpc_reg_rows_table_row   [z_0 | z_1 | z_2 | y] of the spec;  lmpc_reg_rows_table_pad_row: the row no query can reach
//   per query    lmpc_reg_rows_query       q_o per row, sums cleared
//                lmpc_reg_rows_pin         a group of two rows held in scalar registers behind one wait
//                lmpc_reg_rows_group       the group's samples: per row the lane's own sum_f (z_f - q_f)^2, the bandwidth screen, a wave vote,
//                                          and inside the hit branch that row's w m m' (upper triangle) and w y m'
//                lmpc_reg_rows_finish      per row: c0, "no points left", lmpc_reg_rows_solve (Cholesky in place on the row's triangle,
//                                          two triangular solves), the scatter onto (A, B, g) / the workspace record
// One pass over the samples serves all three rows.  The arithmetic per row is lmpc_reg_core.hip.h's with the EXACT weights.
#ifndef LMPC_REG_ROWS_CORE_HIP_H_
#define LMPC_REG_ROWS_CORE_HIP_H_

#include <hip/hip_runtime.h>

#include "lmpc_device.h"
#include "lmpc_reg_rows.h"

#define LMPC_REG_ROWS_UNR 2  // samples per group (tables are padded to a multiple of four, as the one-list tables are)

// One query's state across the sample loop: per row NQ sums of the upper triangle of M'KM, then NM of M'K y.
template <int MF>
struct lmpc_reg_rows_lane {
  static constexpr int NM = MF + 1;
  static constexpr int NQ = NM * (NM + 1) / 2;
  static constexpr int NACC = NQ + NM;
  static constexpr int STRIDE = LMPC_REG_ROWS_STRIDE(MF);
  double q[LMPC_REG_ROWS][MF], nih2;
  double acc[LMPC_REG_ROWS][NACC];
};

// row[o MF + f] = z_o[f], row[3 MF + o] = y[out[o]]; null features and unused rows 0.  (x, u, y are registers: the spec's indices
// select by comparison, not by address.)
__device__ __forceinline__ void lmpc_reg_rows_table_row(const lmpc_reg_rows_dev& spec, const double (&xs)[6], const double (&us)[2],
                                                        const double (&y)[6], double* row) {
  const int mf = spec.mf;
  for (int o = 0; o < LMPC_REG_ROWS; ++o) {
    for (int f = 0; f < mf; ++f) {
      double z = 0.0;
      if (f < spec.nf[o]) {
        const int col = spec.col[o][f];
#pragma unroll
        for (int c = 0; c < 6; ++c) z = col == c ? xs[c] : z;
        z = col == 6 ? us[0] : z;
        z = col == 7 ? us[1] : z;
      }
      row[o * mf + f] = z;
    }
    double yo = 0.0;
    if (o < spec.n_out) {
#pragma unroll
      for (int c = 0; c < 6; ++c) yo = spec.out[o] == c ? y[c] : yo;
    }
    row[LMPC_REG_ROWS * mf + o] = yo;
  }
}

// A padding row: d^2 >= 1e29 for every query of every row (out of every bandwidth, and no 0 * inf in the sums).
__device__ __forceinline__ void lmpc_reg_rows_table_pad_row(const lmpc_reg_rows_dev& spec, double* row) {
  const int mf = spec.mf;
  for (int c = 0; c < LMPC_REG_ROWS_STRIDE(mf); ++c) row[c] = 0.0;
  for (int o = 0; o < LMPC_REG_ROWS; ++o) row[o * mf] = LMPC_REG_ROWS_FAR_Z;
}

// Query (b, i): the linearisation point's features in each row's own space.  A dead lane's query, and the query of a row the spec
// does not use, sit out of every bandwidth.
template <int MF>
__device__ __forceinline__ void lmpc_reg_rows_query(lmpc_reg_rows_lane<MF>& L, const lmpc_reg_rows_dev& spec, int N, int B, int b, int i,
                                                    bool live, const double* __restrict__ X_ref, const double* __restrict__ U_ref) {
  const int NS = N - 1;
#pragma unroll
  for (int o = 0; o < LMPC_REG_ROWS; ++o) {
#pragma unroll
    for (int f = 0; f < MF; ++f) {
      double q = 0.0;
      if (f < spec.nf[o]) {
        const int col = spec.col[o][f];
        q = col < 6 ? X_ref[((size_t)col * N + i) * B + b] : U_ref[((size_t)(col - 6) * NS + i) * B + b];
      }
      L.q[o][f] = q;
    }
    if (!live || o >= spec.n_out) L.q[o][0] = LMPC_REG_ROWS_FAR_Q;
  }
  const double h = spec.dist_max;
  L.nih2 = -1.0 / (h * h);
#pragma unroll
  for (int o = 0; o < LMPC_REG_ROWS; ++o)
#pragma unroll
    for (int a = 0; a < L.NACC; ++a) L.acc[o][a] = 0.0;
}

// Every row of the group is "used" here, in scalar registers, so that the group's scalar loads are issued up front and waited for once
// (lmpc_reg_pin in lmpc_reg_core.hip.h has the measurement; device code only: a host build has no such registers).
template <int MF>
__device__ __forceinline__ void lmpc_reg_rows_pin(double (&row)[LMPC_REG_ROWS_UNR][LMPC_REG_ROWS_STRIDE(MF)]) {
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
  for (int t = 0; t < LMPC_REG_ROWS_UNR; ++t)
#pragma unroll
    for (int c = 0; c < LMPC_REG_ROWS_STRIDE(MF); ++c) asm volatile("" : "+s"(row[t][c]));
#endif
}

// A group of samples (wave-uniform: row[t] = [z_0 | z_1 | z_2 | y] of sample t) against this lane's query.
template <int MF>
__device__ __forceinline__ void lmpc_reg_rows_group(lmpc_reg_rows_lane<MF>& L, const double (&row)[LMPC_REG_ROWS_UNR][LMPC_REG_ROWS_STRIDE(MF)]) {
  constexpr int NM = MF + 1;
  double sq[LMPC_REG_ROWS_UNR][LMPC_REG_ROWS];
#pragma unroll
  for (int t = 0; t < LMPC_REG_ROWS_UNR; ++t)
#pragma unroll
    for (int o = 0; o < LMPC_REG_ROWS; ++o) {
      double s = 0.0;
#pragma unroll
      for (int f = 0; f < MF; ++f) {
        const double df = row[t][o * MF + f] - L.q[o][f];
        s = __builtin_fma(df, df, s);
      }
      // K / c0 = (1 - (d/h)^2)^2 inside the bandwidth, 0 outside (safe_set.cpp:84-87): max(1 - d^2/h^2, 0)^2; c0 = 0.75/h
      // multiplies the sums once, after the loop
      sq[t][o] = fmax(__builtin_fma(s, L.nih2, 1.0), 0.0);
    }
#pragma unroll
  for (int t = 0; t < LMPC_REG_ROWS_UNR; ++t)
#pragma unroll
    for (int o = 0; o < LMPC_REG_ROWS; ++o) {
      if (!__any(sq[t][o] > 0.0)) continue;
      const double w = sq[t][o] * sq[t][o];
      double wm[NM];
#pragma unroll
      for (int r = 0; r < MF; ++r) wm[r] = w * row[t][o * MF + r];
      wm[MF] = w;
      int a = 0;
#pragma unroll
      for (int r = 0; r < NM; ++r)
#pragma unroll
        for (int c = r; c < NM; ++c) {
          L.acc[o][a] += c < MF ? wm[r] * row[t][o * MF + c] : wm[r];
          ++a;
        }
      const double yo = row[t][LMPC_REG_ROWS * MF + o];
#pragma unroll
      for (int r = 0; r < NM; ++r) L.acc[o][a++] += wm[r] * yo;
    }
}

// One row's (MF+1)^2 system: acc = upper triangle of M'KM (NQ, row by row), then M'K y (NM), both already times c0.
// Cholesky of Q = M'KM + 1e-3 I in place on the triangle (U = L', the reciprocal pivots on the diagonal), then L yv = +-b, L' R = yv.
template <int MF>
__device__ __forceinline__ void lmpc_reg_rows_solve(double (&acc)[(MF + 1) * (MF + 2) / 2 + MF + 1], bool negate, double (&R)[MF + 1]) {
  constexpr int NM = MF + 1;
  constexpr int NQ = NM * (NM + 1) / 2;
#define LMPC_RR_U(r, c) acc[(r) * NM - (r) * ((r)-1) / 2 + ((c) - (r))]  // r <= c
#pragma unroll
  for (int jn = 0; jn < NM; ++jn) {
    double dd = LMPC_RR_U(jn, jn) + 1e-3;
#pragma unroll
    for (int k = 0; k < jn; ++k) dd -= LMPC_RR_U(k, jn) * LMPC_RR_U(k, jn);
    const double id = 1.0 / sqrt(dd);
    LMPC_RR_U(jn, jn) = id;
#pragma unroll
    for (int c = jn + 1; c < NM; ++c) {
      double tt = LMPC_RR_U(jn, c);
#pragma unroll
      for (int k = 0; k < jn; ++k) tt -= LMPC_RR_U(k, c) * LMPC_RR_U(k, jn);
      LMPC_RR_U(jn, c) = tt * id;
    }
  }
  double yv[NM];
#pragma unroll
  for (int r = 0; r < NM; ++r) {
    double tt = negate ? -acc[NQ + r] : acc[NQ + r];  // b = M'K y  (as written: -M'K y)
#pragma unroll
    for (int k = 0; k < r; ++k) tt -= LMPC_RR_U(k, r) * yv[k];
    yv[r] = tt * LMPC_RR_U(r, r);
  }
#pragma unroll
  for (int r = NM - 1; r >= 0; --r) {
    double tt = yv[r];
#pragma unroll
    for (int k = r + 1; k < NM; ++k) tt -= LMPC_RR_U(r, k) * R[k];
    R[r] = tt * LMPC_RR_U(r, r);
  }
#undef LMPC_RR_U
}

// Every row's own system, solved and added onto the linearisation of (b, i); a row without a candidate leaves its entries as they are.
// WS_LAYOUT: outA is the linearisation workspace [B][N-1][54] (outB, outg unused); otherwise the A/B/g arrays of lmpc_linearize_batch.
template <int MF, bool WS_LAYOUT>
__device__ __forceinline__ void lmpc_reg_rows_finish(lmpc_reg_rows_lane<MF>& L, const lmpc_reg_rows_dev& spec, int N, int B, int b, int i,
                                                     bool live, double* __restrict__ outA, double* __restrict__ outB,
                                                     double* __restrict__ outg) {
  constexpr int NM = MF + 1;
  constexpr int NQ = NM * (NM + 1) / 2;
  const int NS = N - 1;
  const double c0 = 0.75 / spec.dist_max;
#pragma unroll
  for (int o = 0; o < LMPC_REG_ROWS; ++o) {
    double(&acc)[NQ + NM] = L.acc[o];
#pragma unroll
    for (int a = 0; a < NQ + NM; ++a) acc[a] *= c0;
    // "if there are no points left, skip the regression" (safe_set.cpp:207-210): the weight sum is M'KM's last entry
    if (!live || o >= spec.n_out || !(acc[NQ - 1] > 0.0)) continue;
    double R[NM];
    lmpc_reg_rows_solve<MF>(acc, spec.as_written != 0, R);
    const int rowo = spec.out[o];
#pragma unroll
    for (int f = 0; f < MF; ++f) {
      if (f >= spec.nf[o]) continue;  // a null feature has no column
      const int col = spec.col[o][f];
      if (WS_LAYOUT)
        outA[((size_t)b * NS + i) * LMPC_LIN_RECORD + col * 6 + rowo] += R[f];
      else if (col < 6)
        outA[((size_t)(rowo * 6 + col) * NS + i) * B + b] += R[f];
      else
        outB[((size_t)(rowo * 2 + (col - 6)) * NS + i) * B + b] += R[f];
    }
    if (WS_LAYOUT)
      outA[((size_t)b * NS + i) * LMPC_LIN_RECORD + 48 + rowo] += R[MF];
    else
      outg[((size_t)rowo * NS + i) * B + b] += R[MF];
  }
}

#endif  // LMPC_REG_ROWS_CORE_HIP_H_
