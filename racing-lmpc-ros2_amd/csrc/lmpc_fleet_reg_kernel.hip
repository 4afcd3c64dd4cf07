// lmpc_fleet_reg_kernel.hip -- the error-dynamics regression of lmpc_reg_kernel.hip with query (b, i) run against car b's OWN laps:
// the closed laps in its ring of the fleet safe set (lmpc_fleet_ss.h).  Layout of the tables: lmpc_fleet_reg.h.
//
// What it replaces: SafeSetManager::query(RegQuery) (safe_set.cpp:182-245) called by B controllers on B managers.  The arithmetic
// is lmpc_reg_kernel.hip's, term for term (the header comment there; oracle/regression.py): the last sample of a lap is dropped,
// y_r,j = x_{j+1}[r] - f_d(x_j, u_j, k_j, dt_j)[r] with dt_j = t_{j+1} - t_j (as_written: the reference's literal signs),
// K = 0.75/h (1 - (d/h)^2)^2 for d < h, Q = M'KM + 1e-3 I, one feature list for all rows.
//
// Two kernels, launched back to back in front of every use (lmpc_fleet_reg_launch):
//   lmpc_fleet_reg_pack_kernel, one workgroup per car, gathers the car's samples from the key / xr / aux planes into its dense table,
//     one lmpc_fd per sample for the residual -- but only when the car's ring has changed: the car's lap_count (every crossing and
//     every loaded lap moves it) is compared with the stamp left by the last pack, and an unchanged car's workgroup returns after two
//     loads.  The decision is the device's alone: no host read, no flag from the caller.  A lap closes once in 200 to 400 periods,
//     so the pack is paid then and not every period.  What changes a ring without moving the count on (lmpc_fleet_ss_reset, a load
//     after it, a new spec) sets every stamp to LMPC_FLEET_REG_STALE on the stream (lmpc_capi.hip).
//   lmpc_fleet_regress_kernel<NF, NOUT, WS_LAYOUT>, ONE WAVEFRONT PER (car, chunk of 64 stages), lane = stage.  The wave belongs to
//     one car, so the row address of the sample loop is the same on every lane and the rows still arrive by scalar loads, four
//     samples in flight, as in lmpc_regress_kernel; every lane keeps its own 21 + 6 NOUT (45 + 9 NOUT) sums, factors its own system
//     and adds onto (A, B, g) or the workspace record.  The weight inside the hit branch is always recomputed from sum (z_f - q_f)^2
//     (the EXACT form): the device cannot know whether a car's features are large against the bandwidth.
// Known cost: at N = 20 only 19 of the 64 lanes carry a query -- about 64 / (N - 1) times the lane-instructions of the shared
// kernel per query (profiles/fleet_regression.md); a denser mapping (several cars per wave) would give up the scalar loads.
// No LDS, no cross-lane traffic besides the vote; everything is written with ordinary vector stores.
#include <hip/hip_runtime.h>

#include "lmpc_device.h"
#include "lmpc_dynamics.hip.h"
#include "lmpc_fleet_reg.h"

// One workgroup per car.  Every index below is clamped on the way in (head to a slot, cnt to the ring, a lap's length to the slot),
// so a row of the table is below cap = R (C - 1) rounded up to four whatever the counters in the store say, and v < cap is tested
// once more where it is used.
__global__ __launch_bounds__(256) void lmpc_fleet_reg_pack_kernel(lmpc_fleet_store st, lmpc_vehicle veh, lmpc_regression_spec spec, int cap,
                                                                  double* __restrict__ tab, int* __restrict__ nrow, int* __restrict__ stamp) {
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, nthr = (int)blockDim.x;
  if (b >= st.B) return;
  // (every thread reads the stamp before the barrier below and one thread writes it behind it: the branch is workgroup-uniform)
  const int lc = st.lap_count[b];
  if (stamp[b] == lc) return;
  const int R1 = st.R + 1, C = st.C;
  int head = st.head[b], cnt = st.cnt[b];
  head = head < 0 || head >= R1 ? 0 : head;
  cnt = cnt < 0 ? 0 : (cnt > st.R ? st.R : cnt);
  const int ns = spec.n_in_state, nf = ns + spec.n_in_ctrl, no = spec.n_out, stride = nf + no + 1;
  double* const tb = tab + (size_t)b * (size_t)cap * (size_t)stride;
  int v0 = 0;
  for (int a = 0; a < cnt; ++a) {  // oldest lap first
    int sl = head - cnt + a;
    if (sl < 0) sl += R1;
    const size_t slot = (size_t)b * R1 + sl;
    int n = st.npts[slot];
    n = n < 0 ? 0 : (n > C ? C : n);
    const int m = n > 0 ? n - 1 : 0;  // the last sample of a lap has no successor
    for (int j = tid; j < m; j += nthr) {
      const int v = v0 + j;
      if (v >= cap) break;
      const size_t r = slot * C + j;  // j + 1 < n <= C: the successor is in the slot
      const double2 k0 = st.key[r], k1 = st.key[r + 1];
      double xs[6] = {k0.x, k0.y, 0, 0, 0, 0}, xn[6] = {k1.x, k1.y, 0, 0, 0, 0}, us[2], xp[6];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        xs[2 + c] = st.xr[r * 4 + c];
        xn[2 + c] = st.xr[(r + 1) * 4 + c];
      }
      us[0] = st.aux[r * 4];
      us[1] = st.aux[r * 4 + 1];
      const double kap = st.aux[r * 4 + 2], t0 = st.aux[r * 4 + 3], t1 = st.aux[(r + 1) * 4 + 3];
      lmpc_fd(veh, xs, us, kap, spec.as_written ? t0 - t1 : t1 - t0, xp);
      double y[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) y[c] = xn[c] - xp[c];
      double* row = tb + (size_t)v * stride;
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
      row[nf + no] = s;
    }
    v0 += m;
  }
  const int nv = v0 < cap ? v0 : cap, npad = (nv + 3) & ~3;  // cap is a multiple of four: npad <= cap
  // rows nv .. npad-1: features and residuals 0, |z|^2 = 1e30 (out of every bandwidth, and no 0 * inf in the sums)
  for (int v = nv + tid; v < npad; v += nthr) {
    double* row = tb + (size_t)v * stride;
    for (int c = 0; c < nf + no; ++c) row[c] = 0.0;
    row[nf + no] = 1e30;
  }
  __syncthreads();  // the table is complete (a workgroup's global writes are visible to the kernel launched behind it)
  if (tid == 0) {
    nrow[b] = npad;
    stamp[b] = lc;
  }
}

// WS_LAYOUT: update the linearisation workspace [B][N-1][54]; otherwise the A/B/g arrays of lmpc_linearize_batch.
// grid = B x chunks, chunks = ceil((N - 1) / 64); a dead lane (stage >= N - 1) carries a query out of every bandwidth and stores nothing.
template <int NF, int NOUT, bool WS_LAYOUT>
__global__ __launch_bounds__(64) void lmpc_fleet_regress_kernel(int N, int B, int chunks, lmpc_regression_spec spec, int cap,
                                                                const double* __restrict__ tab, const int* __restrict__ nrow,
                                                                const double* __restrict__ X_ref, const double* __restrict__ U_ref,
                                                                double* __restrict__ outA, double* __restrict__ outB, double* __restrict__ outg) {
  constexpr int NM = NF + 1;
  constexpr int NQ = NM * (NM + 1) / 2;
  constexpr int NROW = NF + NOUT;
  constexpr int STRIDE = NROW + 1;
  constexpr int UNR = 4;
  const int NS = N - 1;
  const int b = (int)blockIdx.x / chunks, ch = (int)blockIdx.x - b * chunks;  // wave-uniform
  if (b >= B) return;
  const int i_lane = ch * 64 + (int)threadIdx.x;
  const bool live = i_lane < NS;
  const int i = live ? i_lane : 0;
  const int ns = spec.n_in_state;
  double q[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f)
    q[f] = f < ns ? X_ref[((size_t)spec.in_state[f] * N + i) * B + b] : U_ref[((size_t)spec.in_ctrl[f - ns] * NS + i) * B + b];
  const double h = spec.dist_max, h2 = h * h, nih2 = -1.0 / h2, c0 = 0.75 / h;
  // the bandwidth screen: d^2 = (|q|^2 + |z|^2) - 2 z.q, one add and NF FMAs per pair with |z|^2 from the row's tail
  double qm2[NF], qq = 0.0;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    if (!live) q[f] = 1e30;
    qm2[f] = -2.0 * q[f];
    qq = __builtin_fma(q[f], q[f], qq);
  }
  double acc[NQ + NOUT * NM];
#pragma unroll
  for (int a = 0; a < NQ + NOUT * NM; ++a) acc[a] = 0.0;
  // this car's table; its padded row count, held inside the table whatever was stored
  const double* __restrict__ tb = tab + (size_t)b * (size_t)cap * (size_t)STRIDE;
  int npad = nrow[b];
  npad = npad < 0 ? 0 : (npad > cap ? cap : npad);
  npad &= ~3;
  for (int j0 = 0; j0 < npad; j0 += UNR) {
    double row[UNR][NROW], zn[UNR], sq[UNR];
#pragma unroll
    for (int t = 0; t < UNR; ++t) {
#pragma unroll
      for (int c = 0; c < NROW; ++c) row[t][c] = tb[(size_t)(j0 + t) * STRIDE + c];  // wave-uniform address: scalar loads
      zn[t] = tb[(size_t)(j0 + t) * STRIDE + NROW];
    }
    // the group's rows are "used" in scalar registers, so that all of them are loaded up front behind one wait (lmpc_reg_kernel.hip;
    // where the group fits the scalar registers: (8, 6) would need 120 of them)
#ifdef __HIP_DEVICE_COMPILE__
    if constexpr (2 * STRIDE * UNR <= 80) {
#pragma unroll
      for (int t = 0; t < UNR; ++t) {
#pragma unroll
        for (int c = 0; c < NROW; ++c) asm volatile("" : "+s"(row[t][c]));
        asm volatile("" : "+s"(zn[t]));
      }
    }
#endif
#pragma unroll
    for (int t = 0; t < UNR; ++t) {
      double s = qq + zn[t];
#pragma unroll
      for (int f = 0; f < NF; ++f) s = __builtin_fma(row[t][f], qm2[f], s);
      sq[t] = fmax(__builtin_fma(s, nih2, 1.0), 0.0);
    }
#pragma unroll
    for (int t = 0; t < UNR; ++t) {
      if (!__any(sq[t] > 0.0)) continue;
      // the weight from sum (z_f - q_f)^2: the expanded form above loses it to cancellation where the features are large against
      // the bandwidth (the abscissa of a 2.8 km lap), and stays the screen.  z_f - q_f from qm2 = -2 q, exactly.
      double s = 0.0;
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const double df = __builtin_fma(qm2[f], 0.5, row[t][f]);
        s = __builtin_fma(df, df, s);
      }
      const double wt = fmax(__builtin_fma(s, nih2, 1.0), 0.0);
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
          acc[a] += c < NF ? wm[r] * row[t][c] : wm[r];
          ++a;
        }
#pragma unroll
      for (int o = 0; o < NOUT; ++o) {
        const double yo = row[t][NF + o];
#pragma unroll
        for (int r = 0; r < NM; ++r) acc[a++] += wm[r] * yo;
      }
    }
  }
#pragma unroll
  for (int a = 0; a < NQ + NOUT * NM; ++a) acc[a] *= c0;
  // "if there are no points left, skip the regression" (safe_set.cpp:207-210): the weight sum is M'KM's last entry.  A car without
  // a closed lap has no rows and leaves its entries as they are.
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

#define LMPC_FLEET_REG_INSTANTIATE(NF, NOUT, WS)                                                                              \
  template __global__ void lmpc_fleet_regress_kernel<NF, NOUT, WS>(int, int, int, lmpc_regression_spec, int, const double*, const int*, \
                                                                   const double*, const double*, double*, double*, double*);
LMPC_FLEET_REG_INSTANTIATE(5, 3, true)
LMPC_FLEET_REG_INSTANTIATE(5, 3, false)
LMPC_FLEET_REG_INSTANTIATE(8, 6, true)
LMPC_FLEET_REG_INSTANTIATE(8, 6, false)

#ifndef LMPC_FLEET_REG_NO_LAUNCHER  // (a host build of the kernels alone defines it)
hipError_t lmpc_fleet_reg_launch(hipStream_t stream, const lmpc_fleet_store& st, const lmpc_vehicle& veh, const lmpc_regression_spec& spec,
                                 const lmpc_fleet_reg_table& tb, int N, bool ws, const double* X_ref, const double* U_ref, double* A,
                                 double* Bm, double* g) {
  hipLaunchKernelGGL(lmpc_fleet_reg_pack_kernel, dim3((unsigned)st.B), dim3(256), 0, stream, st, veh, spec, tb.cap, tb.tab, tb.nrow, tb.stamp);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int chunks = (N - 1 + 63) / 64;
  const dim3 grid((unsigned)st.B * (unsigned)chunks), block(64);
  const bool five = spec.n_in_state + spec.n_in_ctrl == 5;
  const double* tab = tb.tab;
  const int* nrow = tb.nrow;
#define LMPC_FLEET_REG_LAUNCH(NF, NOUT, WS)                                                                                          \
  hipLaunchKernelGGL((lmpc_fleet_regress_kernel<NF, NOUT, WS>), grid, block, 0, stream, N, st.B, chunks, spec, tb.cap, tab, nrow, X_ref, U_ref, A, \
                     Bm, g)
  if (five && ws)
    LMPC_FLEET_REG_LAUNCH(5, 3, true);
  else if (five)
    LMPC_FLEET_REG_LAUNCH(5, 3, false);
  else if (ws)
    LMPC_FLEET_REG_LAUNCH(8, 6, true);
  else
    LMPC_FLEET_REG_LAUNCH(8, 6, false);
#undef LMPC_FLEET_REG_LAUNCH
  return hipGetLastError();
}
#endif
