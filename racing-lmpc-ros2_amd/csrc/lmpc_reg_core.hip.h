// lmpc_reg_core.hip.h -- the error-dynamics regression, once: what lmpc_regress_kernel (lmpc_reg_kernel.hip: one lane per query of
// any car, one shared table) and lmpc_fleet_regress_kernel (lmpc_fleet_reg_kernel.hip: one wavefront per car, the car's own table)
// both do for a lane's query, and what the kernels that build their tables both do for a sample.  The kernels keep how a lane gets
// its (b, i, live) and where a group of rows comes from.  The model, the weights and the history of the loop: lmpc_reg_kernel.hip.
//
//   per sample   lmpc_reg_table_row   [z | y] of the spec and |z|^2;  lmpc_reg_table_pad_row: the row no query can reach
//                (the residual y = x_{j+1} - f_d(x_j, u_j, k_j, +-dt_j) is two lines around lmpc_fd and stays in the two kernels that
//                form it: behind a common function the compiler contracted the last line of the RK4 step, x + dt/6 (...), into an
//                FMA in one kernel or the other where it had not, and y moved by an ulp against the library before)
//   per query    lmpc_reg_query       q -> (-2 q, |q|^2), sums cleared
//                lmpc_reg_pin         a group of four rows held in scalar registers behind one wait
//                lmpc_reg_group       bandwidth screen of the group, then w m m' and w y m' for the rows some lane of the wave is near
//                lmpc_reg_finish      c0, "no points left", Cholesky, the two triangular solves, the scatter onto (A, B, g) / the record
// Everything is __forceinline__ and takes its arrays by reference: after inlining the lane's state is registers, as it was when the
// body stood in the kernel.
#ifndef LMPC_REG_CORE_HIP_H_
#define LMPC_REG_CORE_HIP_H_

#include <hip/hip_runtime.h>

#include "lmpc_device.h"

#define LMPC_REG_UNR 4  // samples per group: tables are padded to a multiple of it

// One query's state across the sample loop: NQ sums of the upper triangle of M'KM, then NOUT x NM of M'K y.
template <int NF, int NOUT>
struct lmpc_reg_lane {
  static constexpr int NM = NF + 1;
  static constexpr int NQ = NM * (NM + 1) / 2;
  static constexpr int NROW = NF + NOUT;
  static constexpr int NACC = NQ + NOUT * NM;
  double qm2[NF], qq, nih2;
  double acc[NACC];
};

// row[0 .. nf) = z = [x[in_state]; u[in_ctrl]], row[nf .. nf + n_out) = y[out]; returns |z|^2.  (x, u, y are registers: the spec's
// indices select by comparison, not by address.)
__device__ __forceinline__ double lmpc_reg_table_row(const lmpc_regression_spec& spec, const double (&xs)[6], const double (&us)[2],
                                                     const double (&y)[6], double* row) {
  const int ns = spec.n_in_state, nf = ns + spec.n_in_ctrl, no = spec.n_out;
  double s = 0.0;
  for (int f = 0; f < nf; ++f) {
    double z = 0.0;
    const int idx = f < ns ? spec.in_state[f] : spec.in_ctrl[f - ns];
    if (f < ns) {
#pragma unroll
      for (int c = 0; c < 6; ++c) z = idx == c ? xs[c] : z;
    } else {
      z = idx == 0 ? us[0] : us[1];
    }
    row[f] = z;
    s = __builtin_fma(z, z, s);
  }
  for (int o = 0; o < no; ++o) {
    double yo = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) yo = spec.out[o] == c ? y[c] : yo;
    row[nf + o] = yo;
  }
  return s;
}

// A padding row: features and residuals 0; returns its |z|^2 = 1e30 (d^2 = 1e30 for every query: out of every bandwidth, and no
// 0 * inf in the sums).
__device__ __forceinline__ double lmpc_reg_table_pad_row(const lmpc_regression_spec& spec, double* row) {
  const int nrow = spec.n_in_state + spec.n_in_ctrl + spec.n_out;
  for (int c = 0; c < nrow; ++c) row[c] = 0.0;
  return 1e30;
}

// Query (b, i): the linearisation point's features.  d^2 = (|q|^2 + |z|^2) - 2 z.q: one add and NF FMAs per pair instead of NF
// subtractions and NF FMAs (|z|^2 comes with the row: it is the same for every lane).  A dead lane's query sits out of every bandwidth.
template <int NF, int NOUT>
__device__ __forceinline__ void lmpc_reg_query(lmpc_reg_lane<NF, NOUT>& L, const lmpc_regression_spec& spec, int N, int B, int b, int i, bool live,
                                               const double* __restrict__ X_ref, const double* __restrict__ U_ref) {
  const int ns = spec.n_in_state, NS = N - 1;
  double q[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f)
    q[f] = f < ns ? X_ref[((size_t)spec.in_state[f] * N + i) * B + b] : U_ref[((size_t)spec.in_ctrl[f - ns] * NS + i) * B + b];
  const double h = spec.dist_max, h2 = h * h;
  L.nih2 = -1.0 / h2;
  L.qq = 0.0;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    if (!live) q[f] = 1e30;
    L.qm2[f] = -2.0 * q[f];
    L.qq = __builtin_fma(q[f], q[f], L.qq);
  }
#pragma unroll
  for (int a = 0; a < L.NACC; ++a) L.acc[a] = 0.0;
}

// Every row of the group is "used" here, in scalar registers: left alone, the compiler loads a sample's features, waits, tests the
// distance, and only inside the hit branch loads its residuals and waits again -- two exposed scalar-cache round trips per sample
// instead of one per group.  (Where the group fits the scalar registers: (8, 6) would need 120 of them.  Device code only: a host
// build of the kernels has no such registers.)
template <int NF, int NOUT>
__device__ __forceinline__ void lmpc_reg_pin(double (&row)[LMPC_REG_UNR][NF + NOUT], double (&zn)[LMPC_REG_UNR]) {
#ifdef __HIP_DEVICE_COMPILE__
  if constexpr (2 * (NF + NOUT + 1) * LMPC_REG_UNR <= 80) {
#pragma unroll
    for (int t = 0; t < LMPC_REG_UNR; ++t) {
#pragma unroll
      for (int c = 0; c < NF + NOUT; ++c) asm volatile("" : "+s"(row[t][c]));
      asm volatile("" : "+s"(zn[t]));
    }
  }
#endif
}

// A group of rows (wave-uniform: row[t] = [z | y] of sample t, zn[t] = |z|^2) against this lane's query.
// EXACT: the features may be large against the bandwidth (the abscissa s of the IAC track runs to 2849 m), where the expanded d^2
// loses the weight to cancellation -- it stays the bandwidth screen, and inside the hit branch each lane recomputes its weight
// from sum_f (z_f - q_f)^2.
template <int NF, int NOUT, bool EXACT>
__device__ __forceinline__ void lmpc_reg_group(lmpc_reg_lane<NF, NOUT>& L, const double (&row)[LMPC_REG_UNR][NF + NOUT],
                                               const double (&zn)[LMPC_REG_UNR]) {
  constexpr int NM = NF + 1;
  double sq[LMPC_REG_UNR];
#pragma unroll
  for (int t = 0; t < LMPC_REG_UNR; ++t) {
    double s = L.qq + zn[t];
#pragma unroll
    for (int f = 0; f < NF; ++f) s = __builtin_fma(row[t][f], L.qm2[f], s);
    // K / c0 = (1 - (d/h)^2)^2 inside the bandwidth, 0 outside (safe_set.cpp:84-87): max(1 - d^2/h^2, 0)^2; c0 = 0.75/h
    // multiplies the sums once, after the loop
    sq[t] = fmax(__builtin_fma(s, L.nih2, 1.0), 0.0);
  }
#pragma unroll
  for (int t = 0; t < LMPC_REG_UNR; ++t) {
    if (!__any(sq[t] > 0.0)) continue;
    double wt = sq[t];
    if constexpr (EXACT) {
      // |q|^2 + |z|^2 - 2 z.q carries a rounding error of a few ulp of |q|^2 + |z|^2 (4e-9 at s = 2849 m against h^2 = 0.36).
      // A sample one form puts inside the bandwidth and the other outside weighs (delta / h^2)^2: negligible either way.
      // (z_f - q_f from qm2 = -2 q, exactly: q itself need not stay live across the loop -- it would take the (8, 6) instance past
      // the 256-VGPR budget and halve its occupancy)
      double s = 0.0;
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const double df = __builtin_fma(L.qm2[f], 0.5, row[t][f]);
        s = __builtin_fma(df, df, s);
      }
      wt = fmax(__builtin_fma(s, L.nih2, 1.0), 0.0);
    }
    const double w = wt * wt;
    double wm[NM];
#pragma unroll
    for (int r = 0; r < NF; ++r) wm[r] = w * row[t][r];
    wm[NF] = w;
    int a = 0;
#pragma unroll
    for (int r = 0; r < NM; ++r)
#pragma unroll
      for (int c = r; c < NM; ++c) {
        L.acc[a] += c < NF ? wm[r] * row[t][c] : wm[r];
        ++a;
      }
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
      const double yo = row[t][NF + o];
#pragma unroll
      for (int r = 0; r < NM; ++r) L.acc[a++] += wm[r] * yo;
    }
  }
}

// The lane's own (NF+1)^2 system, solved and added onto the linearisation of (b, i).
// WS_LAYOUT: outA is the linearisation workspace [B][N-1][54] (outB, outg unused); otherwise the A/B/g arrays of lmpc_linearize_batch.
template <int NF, int NOUT, bool WS_LAYOUT>
__device__ __forceinline__ void lmpc_reg_finish(lmpc_reg_lane<NF, NOUT>& L, const lmpc_regression_spec& spec, int N, int B, int b, int i, bool live,
                                                double* __restrict__ outA, double* __restrict__ outB, double* __restrict__ outg) {
  constexpr int NM = NF + 1;
  constexpr int NQ = NM * (NM + 1) / 2;
  const int ns = spec.n_in_state, NS = N - 1;
  const double c0 = 0.75 / spec.dist_max;
  double(&acc)[NQ + NOUT * NM] = L.acc;
#pragma unroll
  for (int a = 0; a < NQ + NOUT * NM; ++a) acc[a] *= c0;
  // "if there are no points left, skip the regression" (safe_set.cpp:207-210): the weight sum is M'KM's last entry.  (A table
  // without rows -- a car without a closed lap -- leaves its entries as they are.)
  if (!live || !(acc[NQ - 1] > 0.0)) return;
  // Cholesky of Q = M'KM + 1e-3 I, this lane's own system
  double Lc[NM * NM];
  {
    double Q[NM * NM];
    int a = 0;
#pragma unroll
    for (int r = 0; r < NM; ++r)
#pragma unroll
      for (int c = r; c < NM; ++c) {
        Q[r * NM + c] = acc[a] + (r == c ? 1e-3 : 0.0);
        Q[c * NM + r] = Q[r * NM + c];
        ++a;
      }
#pragma unroll
    for (int jn = 0; jn < NM; ++jn) {
      double dd = Q[jn * NM + jn];
#pragma unroll
      for (int k = 0; k < jn; ++k) dd -= Lc[jn * NM + k] * Lc[jn * NM + k];
      const double id = 1.0 / sqrt(dd);
      Lc[jn * NM + jn] = id;  // reciprocal of the pivot
#pragma unroll
      for (int r = jn + 1; r < NM; ++r) {
        double tt = Q[r * NM + jn];
#pragma unroll
        for (int k = 0; k < jn; ++k) tt -= Lc[r * NM + k] * Lc[jn * NM + k];
        Lc[r * NM + jn] = tt * id;
      }
    }
  }
#pragma unroll
  for (int o = 0; o < NOUT; ++o) {
    double yv[NM], R[NM];
#pragma unroll
    for (int r = 0; r < NM; ++r) {
      double tt = spec.as_written ? -acc[NQ + o * NM + r] : acc[NQ + o * NM + r];  // b = M'K y  (as written: -M'K y)
#pragma unroll
      for (int k = 0; k < r; ++k) tt -= Lc[r * NM + k] * yv[k];
      yv[r] = tt * Lc[r * NM + r];
    }
#pragma unroll
    for (int r = NM - 1; r >= 0; --r) {
      double tt = yv[r];
#pragma unroll
      for (int k = r + 1; k < NM; ++k) tt -= Lc[k * NM + r] * R[k];
      R[r] = tt * Lc[r * NM + r];
    }
    const int rowo = spec.out[o];
#pragma unroll
    for (int f = 0; f < NM; ++f) {
      if (f < NF) {
        const int col = f < ns ? spec.in_state[f] : 6 + spec.in_ctrl[f - ns];  // column of [A B]
        if (WS_LAYOUT)
          outA[((size_t)b * NS + i) * LMPC_LIN_RECORD + col * 6 + rowo] += R[f];
        else if (col < 6)
          outA[((size_t)(rowo * 6 + col) * NS + i) * B + b] += R[f];
        else
          outB[((size_t)(rowo * 2 + (col - 6)) * NS + i) * B + b] += R[f];
      } else {
        if (WS_LAYOUT)
          outA[((size_t)b * NS + i) * LMPC_LIN_RECORD + 48 + rowo] += R[f];
        else
          outg[((size_t)rowo * NS + i) * B + b] += R[f];
      }
    }
  }
}

#endif  // LMPC_REG_CORE_HIP_H_
