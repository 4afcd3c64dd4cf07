// lmpc_reg_rows_kernel.hip -- the error-dynamics regression of lmpc_reg_kernel.hip with ONE FEATURE LIST PER REGRESSED ROW
// (lmpc_regression_rows_spec; RegQuery's reg_in_state_idxs / reg_in_control_idxs / reg_out_state_idxs are vectors of vectors,
// safe_set.hpp:61-75): row o of the spec regresses state out[o] on z = [x[S_o]; u[C_o]], with its own distance, candidates, weights
// and (|S_o| + |C_o| + 1)^2 system.  The model, the reading of the reference and the two sign conventions: lmpc_reg_kernel.hip.
//
// Two kernels.  Once per lap upload lmpc_reg_rows_pack_kernel gathers the samples that have a successor (residuals from
// lmpc_reg_residual_kernel, as for the one-list form) into one dense table in the PACKED PER-ROW layout
//   tab[v] = [ z_0 (MF) | z_1 (MF) | z_2 (MF) | y_0 y_1 y_2 ],   120 bytes per sample for MF = 4, 144 for MF = 5
// (lmpc_reg_rows.h), padded to a multiple of four with rows no query can reach.  Packed and not [x u | y] with selects: every
// operand of the sample loop is then a scalar register named at compile time, and a list shorter than MF costs FMAs with 0, not
// selects; a null feature decouples exactly.  Per solve lmpc_regress_rows_kernel<MF, WS_LAYOUT> follows lmpc_regress_kernel: one
// lane per query (problem, stage), the sample loop wave-uniform, a sample's row by scalar loads, no cross-lane reduction, no
// per-lane gather, no LDS, results by ordinary vector stores.  TWO samples per group, not four: a group is held in scalar registers
// behind one wait (lmpc_reg_rows_pin), and two rows of 30 / 36 registers are what fits beside the spec -- four samples without the pin
// compiled to ten waits per group, and a one-row spec then cost what three rows cost (3.42 against 3.35 ms on the shape below: the
// loop waited for the scalar cache, not for the FP64 pipe); pinned pairs: 2.16 against 3.28 ms.  ONE pass over the samples serves all three
// rows: per sample and row the lane's own sum_f (z_f - q_f)^2 (always the direct form -- three norms per sample leave the expanded
// form's |z|^2 column nothing to save), max(1 - d^2/h^2, 0), a wave vote, and inside the hit branch that row's 21 (15) sums of
// w m m' and 6 (5) of w y m' for MF = 5 (4).  Fewer than three rows: the missing rows are null and their query is out of reach.
// Two instances per layout, MF = 4 and MF = 5; the longest list of the spec decides.
// Resources (gfx950, __launch_bounds__(64), -Rpass-analysis=kernel-resource-usage on the unity build), array / workspace layout:
//   MF = 4   163 VGPRs, 106 SGPRs, no scratch, 3 waves / SIMD;   per-car kernel 161 VGPRs
//   MF = 5   213 VGPRs, 106 SGPRs, no scratch, 2 waves / SIMD;   per-car kernel 211 VGPRs
// No VGPR is spilled; 18 .. 48 SGPRs are (to VGPR lanes, v_writelane / v_readlane), all of them in the query set-up and the scatter,
// which hold the spec's thirty indices -- the sample loop has none: per group of two samples 235 (MF = 4) / 295 (MF = 5) instructions
// with all three rows inside the hit branch, five s_load and one s_waitcnt among them; 108 / 138 VALU instructions per (sample, lane),
// 33 / 39 of them the three distances and screens that every sample pays.  Measured (MI355X, 32768 x 19 queries, 2200 samples,
// bench.py's config-5 shape): 3.28 ms for three 4-feature lists, 4.31 ms for three 5-feature lists, against 1.52 ms of the one-list
// (5, 3) kernel and 6.48 ms for three one-row passes of the 4-feature lists (profiles/regression_rows.md).
#include <hip/hip_runtime.h>

#include "lmpc_device.h"
#include "lmpc_reg_rows_core.hip.h"

// tab[v][3 MF + 3] for the valid samples (valid[v] = index of a sample that is not the last of its lap), v < nvalid;
// rows nvalid .. npad-1: padding rows
__global__ void lmpc_reg_rows_pack_kernel(lmpc_reg_rows_dev spec, int nvalid, int npad, const int* __restrict__ valid,
                                          const double* __restrict__ x, const double* __restrict__ u, const double* __restrict__ y,
                                          double* __restrict__ tab) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= npad) return;
  double* row = tab + (size_t)v * LMPC_REG_ROWS_STRIDE(spec.mf);
  if (v >= nvalid) {
    lmpc_reg_rows_table_pad_row(spec, row);
    return;
  }
  const int j = valid[v];
  double xs[6], ys[6], us[2];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    xs[c] = x[(size_t)j * 6 + c];
    ys[c] = y[(size_t)j * 6 + c];
  }
  us[0] = u[(size_t)j * 2];
  us[1] = u[(size_t)j * 2 + 1];
  lmpc_reg_rows_table_row(spec, xs, us, ys, row);
}

// One lane per query (b, i) of any car, 64 queries per wave; the table is tab with row stride 3 MF + 3.
// WS_LAYOUT: update the handle's linearisation workspace [B][N-1][54]; otherwise the A/B/g arrays of lmpc_linearize_batch.
template <int MF, bool WS_LAYOUT>
__global__ __launch_bounds__(64) void lmpc_regress_rows_kernel(int N, int B, lmpc_reg_rows_dev spec, int npad, const double* __restrict__ tab,
                                                               const double* __restrict__ X_ref, const double* __restrict__ U_ref,
                                                               double* __restrict__ outA, double* __restrict__ outB,
                                                               double* __restrict__ outg) {
  constexpr int STRIDE = LMPC_REG_ROWS_STRIDE(MF);
  constexpr int UNR = LMPC_REG_ROWS_UNR;
  const int NS = N - 1;
  const long long gq = (long long)blockIdx.x * 64 + threadIdx.x;
  const bool live = gq < (long long)B * NS;
  const long long gqc = live ? gq : 0;
  const int b = (int)(gqc / NS), i = (int)(gqc - (long long)b * NS);
  lmpc_reg_rows_lane<MF> L;
  lmpc_reg_rows_query(L, spec, N, B, b, i, live, X_ref, U_ref);
  for (int j0 = 0; j0 < npad; j0 += UNR) {
    double row[UNR][STRIDE];
#pragma unroll
    for (int t = 0; t < UNR; ++t)
#pragma unroll
      for (int c = 0; c < STRIDE; ++c) row[t][c] = tab[(size_t)(j0 + t) * STRIDE + c];  // wave-uniform address: scalar loads
    lmpc_reg_rows_pin<MF>(row);
    lmpc_reg_rows_group<MF>(L, row);
  }
  lmpc_reg_rows_finish<MF, WS_LAYOUT>(L, spec, N, B, b, i, live, outA, outB, outg);
}

#define LMPC_REG_ROWS_INSTANTIATE(MF, WS)                                                                                          \
  template __global__ void lmpc_regress_rows_kernel<MF, WS>(int, int, lmpc_reg_rows_dev, int, const double*, const double*, const double*, \
                                                            double*, double*, double*);
LMPC_REG_ROWS_INSTANTIATE(4, true)
LMPC_REG_ROWS_INSTANTIATE(4, false)
LMPC_REG_ROWS_INSTANTIATE(5, true)
LMPC_REG_ROWS_INSTANTIATE(5, false)
