// lmpc_dtrack_model_kernel.hip -- lmpc_linearize_dtrack_kernel: the discrete Jacobian (A, Bm, g) of the DOUBLE-TRACK planar model for
// every stage of every problem, problem b linearised on vehicle b of the handle's double-track table (include/lmpc_hip_dtrack_model.h).
// It writes what lmpc_linearize_kernel (lmpc_prep_kernels.hip) writes, in the same layouts, so every QP kernel behind it runs on the
// four-wheel model unchanged.
//
// The map that is linearised: Phi(x, u; k, dt) = out(step_native(in(x), u, k, dt)) in the plant layout x = [s, e_y, e_psi, vx, vy, omega],
// u = [LON, STEER] -- `in` and `out` are the conversions of lmpc_hip_dtrack.h decision 2, the controls are mapped by decision 3 --, ONE
// step of dt = T_ref[i][b] with u and k = curvatures[i][b] held: RK4, or Euler where vehicle b's integrator says so.  No curvature
// lookup, no abscissa wrap, no sub-steps: those are the plant's.  The speed guard is applied once, on entry: where hypot(vx, vy) < 1e-6
// the evaluation uses v = 1e-6, for the value and in the derivatives of `in` (d v = 0, d beta = (vx d vy - vy d vx) / 1e-12), so the
// outputs there are finite.
//
// One lane per (problem b, stage i), blockIdx.y = stage: lmpc_linearize_kernel's grid, its coalesced [field][knot][batch] loads and
// its stores.  A lane loads its vehicle (34 coalesced loads of 8 bytes and one of 4).  The primal sweep over the four RK4 points keeps
// the partials of the continuous dynamics in the native state (csrc/lmpc_dtrack_partials.hip.h): five numbers for the kinematic rows
// and 3 x 5 for the force block, whose five tangents travel together through the tyres and the implicit load transfer.  The eight
// columns of [A Bm] are then pushed through one at a time (`unroll 1`, as lmpc_linearize_kernel), each seeded with a column of the
// Jacobian of `in` and closed with the Jacobian of `out`.  No LDS, no barrier, no cross-lane operation; a lane past the batch returns
// before it reads anything.  256 VGPRs + 208 AGPRs at one wave per SIMD, no scratch.
//
// A translation unit of its own (csrc/Makefile): the kernel and its launcher, called from lmpc_capi.hip through lmpc_dtrack_model.h.
#include <hip/hip_runtime.h>

#include "lmpc_device.h"  // LMPC_LIN_RECORD
#include "lmpc_dtrack_model.h"
#include "lmpc_dtrack_partials.hip.h"

// the value of x materialised in a vector register at this point of the program (an empty statement: no instruction is emitted)
#define LMPC_DTM_PIN(x) asm volatile("" : "+v"(x))

template <bool WS_LAYOUT>
__global__ __launch_bounds__(256, 1) void lmpc_linearize_dtrack_kernel(const double* __restrict__ tab, int N, int B,
                                                                    const double* __restrict__ X_ref, const double* __restrict__ U_ref,
                                                                    const double* __restrict__ T_ref, const double* __restrict__ curv,
                                                                    double* __restrict__ outA, double* __restrict__ outB,
                                                                    double* __restrict__ outg) {
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
  lmpc_vehicle_dt veh;
  dtrack_vehicle(tab, B, b, veh);
  const bool euler = veh.base.integrator == LMPC_INTEGRATOR_EULER;

  dtm_uterms ut;
  dtm_u_terms(veh.base, u[0], u[1], ut);
  // `in`: [s, e_y, e_psi, vx, vy, omega] -> [s, e_y, e_psi, omega, beta, v], and its two non-trivial columns
  const double r2 = x[3] * x[3] + x[4] * x[4];
  double z[6] = {x[0], x[1], x[2], x[5], atan2(x[4], x[3]), hypot(x[3], x[4])};
  const bool guard = z[5] < 1e-6;
  if (guard) z[5] = 1e-6;
  const double r2g = guard ? 1e-12 : r2;
  const double in_beta[2] = {-x[4] / r2g, x[3] / r2g};                              // d beta / d vx, / d vy
  const double in_v[2] = {guard ? 0.0 : x[3] / z[5], guard ? 0.0 : x[4] / z[5]};  // d v / d vx, / d vy

  // weights of the four slopes: dt/6 (1, 2, 2, 1), or the first slope alone (Euler, utils.cpp:110-123), as lmpc_linearize_kernel
  const double wgt[4] = {euler ? dt : dt / 6, euler ? 0.0 : dt / 3, euler ? 0.0 : dt / 3, euler ? 0.0 : dt / 6};
  // the primal sweep: the four slopes, summed as they come, and the partials at their points
  dtm_kin Jk[4];
  double Jf[4][3][5], kprev[6], z1[6], zs[6];
  const double cs[4] = {0.0, 0.5, 0.5, 1.0};
#pragma unroll
  for (int s = 0; s < 4; ++s) {
#pragma unroll
    for (int r = 0; r < 6; ++r) zs[r] = (s == 0) ? z[r] : z[r] + cs[s] * dt * kprev[r];
    dtm_kinematics(zs, kap, kprev, Jk[s]);
    dtm_dual<5> f[3];
    dtm_force<5>(veh, ut, zs[3], zs[4], zs[5], 0, f);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      kprev[3 + r] = f[r].v;
#pragma unroll
      for (int j = 0; j < 5; ++j) Jf[s][r][j] = f[r].d[j];
    }
    // What the point leaves behind -- 5 + 15 partials and the slope -- is FINISHED here, each value pinned in a register.  Left to
    // itself the compiler puts off the last operations of the partials until the column loop needs them and keeps their operands
    // alive instead, 80 doubles per point where the partials are 20: 256 + 256 registers and 1092 bytes of scratch per lane.
    // Pinned: 256 VGPRs + 208 AGPRs, no scratch, the same arithmetic.
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int j = 0; j < 5; ++j) LMPC_DTM_PIN(Jf[s][r][j]);
    }
    LMPC_DTM_PIN(Jk[s].f0_ey);
    LMPC_DTM_PIN(Jk[s].f0_ang);
    LMPC_DTM_PIN(Jk[s].f0_v);
    LMPC_DTM_PIN(Jk[s].f1_ang);
    LMPC_DTM_PIN(Jk[s].f1_v);
#pragma unroll
    for (int r = 0; r < 6; ++r) LMPC_DTM_PIN(kprev[r]);
#pragma unroll
    for (int r = 0; r < 6; ++r) z1[r] = (s == 0) ? z[r] + wgt[0] * kprev[r] : z1[r] + wgt[s] * kprev[r];
  }
  // `out`: vx = v cos(beta), vy = v sin(beta)
  double sb1, cb1;
  sincos(z1[4], &sb1, &cb1);
  double gacc[6] = {z1[0], z1[1], z1[2], z1[5] * cb1, z1[5] * sb1, z1[3]};

#pragma unroll 1
  for (int c = 0; c < 8; ++c) {
    // column c of the Jacobian of `in` (native tangent) and of the controls
    const double tu[2] = {c == 6 ? 1.0 : 0.0, c == 7 ? 1.0 : 0.0};
    double e[6], tz[6], kc[6], acc[6];
    e[0] = (c == 0) ? 1.0 : 0.0;
    e[1] = (c == 1) ? 1.0 : 0.0;
    e[2] = (c == 2) ? 1.0 : 0.0;
    e[3] = (c == 5) ? 1.0 : 0.0;
    e[4] = (c == 3) ? in_beta[0] : ((c == 4) ? in_beta[1] : 0.0);
    e[5] = (c == 3) ? in_v[0] : ((c == 4) ? in_v[1] : 0.0);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      tz[r] = e[r];
      acc[r] = 0.0;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const double ang = tz[2] + tz[4];
      kc[0] = Jk[s].f0_ey * tz[1] + Jk[s].f0_ang * ang + Jk[s].f0_v * tz[5];
      kc[1] = Jk[s].f1_ang * ang + Jk[s].f1_v * tz[5];
      kc[2] = tz[3] - kap * kc[0];
#pragma unroll
      for (int r = 0; r < 3; ++r)
        kc[3 + r] = Jf[s][r][0] * tz[3] + Jf[s][r][1] * tz[4] + Jf[s][r][2] * tz[5] + Jf[s][r][3] * tu[0] + Jf[s][r][4] * tu[1];
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        acc[r] += wgt[s] * kc[r];
        if (s < 3) tz[r] = e[r] + cs[s + 1] * dt * kc[r];
      }
    }
    // the native tangent of the step, through the Jacobian of `out`
    double t1[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) t1[r] = e[r] + acc[r];
    const double d[6] = {t1[0], t1[1], t1[2], t1[5] * cb1 - z1[5] * sb1 * t1[4], t1[5] * sb1 + z1[5] * cb1 * t1[4], t1[3]};
    // x[c] / u[c - 6], read again (c is a run-time index: one load instead of eight live values and a chain of selects)
    const double xu = (c < 6) ? X_ref[(size_t)(c * N + i) * B + b] : U_ref[(size_t)((c - 6) * NS + i) * B + b];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      gacc[r] -= d[r] * xu;  // [A Bm][r][c]
      if (WS_LAYOUT)
        outA[((size_t)b * NS + i) * LMPC_LIN_RECORD + c * 6 + r] = d[r];
      else if (c < 6)
        outA[((size_t)(r * 6 + c) * NS + i) * B + b] = d[r];
      else
        outB[((size_t)(r * 2 + (c - 6)) * NS + i) * B + b] = d[r];
    }
  }
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    if (WS_LAYOUT)
      outA[((size_t)b * NS + i) * LMPC_LIN_RECORD + 48 + r] = gacc[r];
    else
      outg[((size_t)r * NS + i) * B + b] = gacc[r];
  }
}

#undef LMPC_DTM_PIN

hipError_t lmpc_dtrack_launch_linearize(hipStream_t stream, const double* tab, int N, int B, bool ws, const double* X_ref, const double* U_ref,
                                        const double* T_ref, const double* curv, double* A, double* Bm, double* g) {
  const dim3 grid((B + 255) / 256, N - 1);
  if (ws)
    hipLaunchKernelGGL(lmpc_linearize_dtrack_kernel<true>, grid, dim3(256), 0, stream, tab, N, B, X_ref, U_ref, T_ref, curv, A, Bm, g);
  else
    hipLaunchKernelGGL(lmpc_linearize_dtrack_kernel<false>, grid, dim3(256), 0, stream, tab, N, B, X_ref, U_ref, T_ref, curv, A, Bm, g);
  return hipGetLastError();
}
