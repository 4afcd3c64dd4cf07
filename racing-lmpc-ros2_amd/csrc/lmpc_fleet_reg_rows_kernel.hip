// lmpc_fleet_reg_rows_kernel.hip -- the per-car error-dynamics regression of lmpc_fleet_reg_kernel.hip with one feature list per
// regressed row (lmpc_regression_rows_spec): query (b, i) regresses every row of the spec, each in its own feature space, on car b's
// OWN closed laps.  Included by lmpc_fleet_reg_kernel.hip: the same translation unit.  The arithmetic is lmpc_reg_rows_core.hip.h,
// which lmpc_reg_rows_kernel.hip runs on the shared store; the table's row is lmpc_reg_rows.h's, 3 MF + 3 doubles with no |z|^2
// column: tab [car][cap][3 MF + 3], nrow and stamp as in lmpc_fleet_reg.h.
//
// Two kernels, launched back to back in front of every use (lmpc_fleet_reg_rows_launch), as in the one-list form:
//   lmpc_fleet_reg_rows_pack_kernel, one workgroup per car: the stamp logic and the gather of lmpc_fleet_reg_pack_kernel -- a car is
//     packed only when its lap_count has moved since its last pack -- writing rows of the per-row layout.
//   lmpc_fleet_regress_rows_kernel<MF, WS_LAYOUT>, one wavefront per (car, chunk of 64 stages), lane = stage: the rows of the car's
//     table by scalar loads, two samples per group behind one wait, one pass for all three rows, every lane its own sums and systems.
// No LDS, no cross-lane traffic besides the votes; everything is written with ordinary vector stores.
#include <hip/hip_runtime.h>

#include "lmpc_device.h"
#include "lmpc_dynamics.hip.h"
#include "lmpc_fleet_reg.h"
#include "lmpc_reg_rows_core.hip.h"

// One workgroup per car.  Every index below is clamped on the way in (head to a slot, cnt to the ring, a lap's length to the slot),
// so a row of the table is below cap = R (C - 1) rounded up to four whatever the counters in the store say, and v < cap is tested
// once more where it is used.
__global__ __launch_bounds__(256) void lmpc_fleet_reg_rows_pack_kernel(lmpc_fleet_store st, lmpc_vehicle veh, lmpc_reg_rows_dev spec, int cap,
                                                                       double* __restrict__ tab, int* __restrict__ nrow,
                                                                       int* __restrict__ stamp) {
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, nthr = (int)blockDim.x;
  if (b >= st.B) return;
  // (every thread reads the stamp before the barrier below and one thread writes it behind it: the branch is workgroup-uniform)
  const int lc = st.lap_count[b];
  if (stamp[b] == lc) return;
  const int R1 = st.R + 1, C = st.C;
  int head = st.head[b], cnt = st.cnt[b];
  head = head < 0 || head >= R1 ? 0 : head;
  cnt = cnt < 0 ? 0 : (cnt > st.R ? st.R : cnt);
  const int stride = LMPC_REG_ROWS_STRIDE(spec.mf);
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
      lmpc_reg_rows_table_row(spec, xs, us, y, tb + (size_t)v * stride);
    }
    v0 += m;
  }
  const int nv = v0 < cap ? v0 : cap, npad = (nv + 3) & ~3;  // cap is a multiple of four: npad <= cap
  for (int v = nv + tid; v < npad; v += nthr) lmpc_reg_rows_table_pad_row(spec, tb + (size_t)v * stride);  // rows nv .. npad-1
  __syncthreads();  // the table is complete (a workgroup's global writes are visible to the kernel launched behind it)
  if (tid == 0) {
    nrow[b] = npad;
    stamp[b] = lc;
  }
}

// WS_LAYOUT: update the linearisation workspace [B][N-1][54]; otherwise the A/B/g arrays of lmpc_linearize_batch.
// grid = B x chunks, chunks = ceil((N - 1) / 64); a dead lane (stage >= N - 1) carries a query out of every bandwidth and stores nothing.
template <int MF, bool WS_LAYOUT>
__global__ __launch_bounds__(64) void lmpc_fleet_regress_rows_kernel(int N, int B, int chunks, lmpc_reg_rows_dev spec, int cap,
                                                                     const double* __restrict__ tab, const int* __restrict__ nrow,
                                                                     const double* __restrict__ X_ref, const double* __restrict__ U_ref,
                                                                     double* __restrict__ outA, double* __restrict__ outB,
                                                                     double* __restrict__ outg) {
  constexpr int STRIDE = LMPC_REG_ROWS_STRIDE(MF);
  constexpr int UNR = LMPC_REG_ROWS_UNR;
  const int NS = N - 1;
  const int b = (int)blockIdx.x / chunks, ch = (int)blockIdx.x - b * chunks;  // wave-uniform
  if (b >= B) return;
  const int i_lane = ch * 64 + (int)threadIdx.x;
  const bool live = i_lane < NS;
  const int i = live ? i_lane : 0;
  lmpc_reg_rows_lane<MF> L;
  lmpc_reg_rows_query(L, spec, N, B, b, i, live, X_ref, U_ref);
  // this car's table; its padded row count, held inside the table whatever was stored
  const double* __restrict__ tb = tab + (size_t)b * (size_t)cap * (size_t)STRIDE;
  int npad = nrow[b];
  npad = npad < 0 ? 0 : (npad > cap ? cap : npad);
  npad &= ~3;
  for (int j0 = 0; j0 < npad; j0 += UNR) {
    double row[UNR][STRIDE];
#pragma unroll
    for (int t = 0; t < UNR; ++t)
#pragma unroll
      for (int c = 0; c < STRIDE; ++c) row[t][c] = tb[(size_t)(j0 + t) * STRIDE + c];  // wave-uniform address: scalar loads
    lmpc_reg_rows_pin<MF>(row);
    lmpc_reg_rows_group<MF>(L, row);
  }
  lmpc_reg_rows_finish<MF, WS_LAYOUT>(L, spec, N, B, b, i, live, outA, outB, outg);
}

#define LMPC_FLEET_REG_ROWS_INSTANTIATE(MF, WS)                                                                                          \
  template __global__ void lmpc_fleet_regress_rows_kernel<MF, WS>(int, int, int, lmpc_reg_rows_dev, int, const double*, const int*, const double*, \
                                                                  const double*, double*, double*, double*);
LMPC_FLEET_REG_ROWS_INSTANTIATE(4, true)
LMPC_FLEET_REG_ROWS_INSTANTIATE(4, false)
LMPC_FLEET_REG_ROWS_INSTANTIATE(5, true)
LMPC_FLEET_REG_ROWS_INSTANTIATE(5, false)

#ifndef LMPC_FLEET_REG_NO_LAUNCHER  // (a host build of the kernels alone defines it)
hipError_t lmpc_fleet_reg_rows_launch(hipStream_t stream, const lmpc_fleet_store& st, const lmpc_vehicle& veh, const lmpc_reg_rows_dev& spec,
                                      const lmpc_fleet_reg_table& tb, int N, bool ws, const double* X_ref, const double* U_ref, double* A,
                                      double* Bm, double* g) {
  hipLaunchKernelGGL(lmpc_fleet_reg_rows_pack_kernel, dim3((unsigned)st.B), dim3(256), 0, stream, st, veh, spec, tb.cap, tb.tab, tb.nrow,
                     tb.stamp);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int chunks = (N - 1 + 63) / 64;
  const dim3 grid((unsigned)st.B * (unsigned)chunks), block(64);
  const double* tab = tb.tab;
  const int* nrow = tb.nrow;
#define LMPC_FLEET_REG_ROWS_LAUNCH(MF, WS)                                                                                             \
  hipLaunchKernelGGL((lmpc_fleet_regress_rows_kernel<MF, WS>), grid, block, 0, stream, N, st.B, chunks, spec, tb.cap, tab, nrow, X_ref, U_ref, A, \
                     Bm, g)
  if (spec.mf == 4 && ws)
    LMPC_FLEET_REG_ROWS_LAUNCH(4, true);
  else if (spec.mf == 4)
    LMPC_FLEET_REG_ROWS_LAUNCH(4, false);
  else if (ws)
    LMPC_FLEET_REG_ROWS_LAUNCH(5, true);
  else
    LMPC_FLEET_REG_ROWS_LAUNCH(5, false);
#undef LMPC_FLEET_REG_ROWS_LAUNCH
  return hipGetLastError();
}
#endif
