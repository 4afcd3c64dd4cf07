// lmpc_cars_model_kernel.hip -- lmpc_linearize_cars_kernel: the discrete Jacobian (A, Bm, g) of the single-track planar model for every
// stage of every problem, problem b linearised on vehicle b of the handle's CAR TABLE (include/lmpc_hip_cars_model.h).  It writes what
// lmpc_linearize_kernel (lmpc_prep_kernels.hip) writes, in the same layouts, from the same model text -- lmpc_u_terms, lmpc_f<true> and
// lmpc_jvp of lmpc_dynamics.hip.h --, so every QP kernel behind it runs on each car's own vehicle unchanged.  The one difference: where
// that kernel reads P.veh, a kernel argument that lives in scalar registers, lane (b, i) here takes its lmpc_vehicle from the table
// through lmpc_car_vehicle (csrc/lmpc_cars.h), into vector registers.
//
// One lane per (problem b, stage i), blockIdx.y = stage: lmpc_linearize_kernel's grid, its coalesced [field][knot][batch] loads and its
// stores.  The table loads are issued with the loads of the linearisation point, ahead of the dynamics, so that all of them are in
// flight at once; lmpc_car_vehicle names all 25 doubles, and the seven the dynamics never read (b, Fd_max, Fb_max, Td, Tb, max_steer,
// max_steer_rate) are never loaded: a load whose value nothing uses is not emitted.  What depends on the vehicle alone (lr, lf, h / l,
// the drag and downforce factors, the static loads) is derived once per lane: lmpc_f is inlined four times and the common
// subexpressions are shared.  Car b's own integrator picks the weights of the four slopes.  The primal sweep over the four RK4 points
// and the `unroll 1` column loop are lmpc_linearize_kernel's.  No LDS, no barrier, no cross-lane operation, ordinary vector stores; a
// lane past the batch returns before it reads anything.  One wave per SIMD (DESIGN.md section 4 has the resource line).
//
// A translation unit of its own (csrc/Makefile): the kernel and its launchers, called from lmpc_capi.hip through lmpc_cars_model.h.
#include <hip/hip_runtime.h>

#include "lmpc_cars_model.h"
#include "lmpc_device.h"  // LMPC_LIN_RECORD
#include "lmpc_dynamics.hip.h"

// io = element type of the arrays (double, or float for the single-precision solve); the arithmetic is fp64.
template <bool WS_LAYOUT, typename io>
__global__ __launch_bounds__(256, 1) void lmpc_linearize_cars_kernel(const double* __restrict__ tab, int N, int B,
                                                                  const io* __restrict__ X_ref, const io* __restrict__ U_ref,
                                                                  const io* __restrict__ T_ref, const io* __restrict__ curv,
                                                                  io* __restrict__ outA, io* __restrict__ outB, io* __restrict__ outg) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = blockIdx.y;
  const int NS = N - 1;
  if (b >= B) return;
  double x[6], u[2];
#pragma unroll
  for (int k = 0; k < 6; ++k) x[k] = X_ref[(size_t)(k * N + i) * B + b];
#pragma unroll
  for (int k = 0; k < 2; ++k) u[k] = U_ref[(size_t)(k * NS + i) * B + b];
  const double dt = T_ref[(size_t)i * B + b];
  const double kap = curv[(size_t)i * B + b];
  lmpc_vehicle veh;
  lmpc_car_vehicle(tab, B, b, veh);

  lmpc_uterms ut;
  lmpc_u_terms(veh, u[0], u[1], ut);
  lmpc_fjac J[4];
  double ks[4][6], xs[6];
  const double cs[4] = {0.0, 0.5, 0.5, 1.0};
#pragma unroll
  for (int s = 0; s < 4; ++s) {
#pragma unroll
    for (int r = 0; r < 6; ++r) xs[r] = (s == 0) ? x[r] : x[r] + cs[s] * dt * ks[s - 1][r];
    lmpc_f<true>(veh, ut, xs, kap, ks[s], &J[s]);
  }
  // weights of the four slopes: dt/6 (1, 2, 2, 1), or the first slope alone where car b integrates with Euler (utils.cpp:110-123)
  const bool euler = veh.integrator == LMPC_INTEGRATOR_EULER;
  const double wgt[4] = {euler ? dt : dt / 6, euler ? 0.0 : dt / 3, euler ? 0.0 : dt / 3, euler ? 0.0 : dt / 6};
  double xp[6], gacc[6];
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    xp[r] = x[r] + (wgt[0] * ks[0][r] + wgt[1] * ks[1][r] + wgt[2] * ks[2][r] + wgt[3] * ks[3][r]);
    gacc[r] = xp[r];
  }
  // one column at a time, as lmpc_linearize_kernel: unrolled, the eight columns' chains are interleaved and the register set doubles
#pragma unroll 1
  for (int c = 0; c < 8; ++c) {
    double tu[2] = {c == 6 ? 1.0 : 0.0, c == 7 ? 1.0 : 0.0};
    double e[6], tx[6], kc[6], acc[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      e[r] = (r == c) ? 1.0 : 0.0;
      tx[r] = e[r];
      acc[r] = 0.0;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      lmpc_jvp(J[s], tx, tu, kc);
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        acc[r] += wgt[s] * kc[r];
        if (s < 3) tx[r] = e[r] + cs[s + 1] * dt * kc[r];
      }
    }
    double xu = x[0];  // (x[c] / u[c - 6] by selects: c is a run-time index, and an indexed register array would live in scratch)
#pragma unroll
    for (int k = 1; k < 6; ++k) xu = (c == k) ? x[k] : xu;
    xu = (c == 6) ? u[0] : ((c == 7) ? u[1] : xu);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const double d = e[r] + acc[r];  // [A B][r][c]
      gacc[r] -= d * xu;
      if (WS_LAYOUT)
        outA[((size_t)b * NS + i) * LMPC_LIN_RECORD + c * 6 + r] = (io)d;
      else if (c < 6)
        outA[((size_t)(r * 6 + c) * NS + i) * B + b] = (io)d;
      else
        outB[((size_t)(r * 2 + (c - 6)) * NS + i) * B + b] = (io)d;
    }
  }
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    if (WS_LAYOUT)
      outA[((size_t)b * NS + i) * LMPC_LIN_RECORD + 48 + r] = (io)gacc[r];
    else
      outg[((size_t)r * NS + i) * B + b] = (io)gacc[r];
  }
}

hipError_t lmpc_cars_launch_linearize(hipStream_t stream, const double* tab, int N, int B, bool ws, const double* X_ref, const double* U_ref,
                                      const double* T_ref, const double* curv, double* A, double* Bm, double* g) {
  const dim3 grid((B + 255) / 256, N - 1);
  if (ws)
    hipLaunchKernelGGL((lmpc_linearize_cars_kernel<true, double>), grid, dim3(256), 0, stream, tab, N, B, X_ref, U_ref, T_ref, curv, A, Bm, g);
  else
    hipLaunchKernelGGL((lmpc_linearize_cars_kernel<false, double>), grid, dim3(256), 0, stream, tab, N, B, X_ref, U_ref, T_ref, curv, A, Bm, g);
  return hipGetLastError();
}

hipError_t lmpc_cars_launch_linearize_f32(hipStream_t stream, const double* tab, int N, int B, const float* X_ref, const float* U_ref,
                                          const float* T_ref, const float* curv, float* ws) {
  const dim3 grid((B + 255) / 256, N - 1);
  hipLaunchKernelGGL((lmpc_linearize_cars_kernel<true, float>), grid, dim3(256), 0, stream, tab, N, B, X_ref, U_ref, T_ref, curv, ws,
                     (float*)nullptr, (float*)nullptr);
  return hipGetLastError();
}
