// lmpc_ekf_kernel.hip -- gfx950 kernels of the batched extended Kalman filter (csrc/lmpc_ekf.h): one thread per car, the batch axis
// on the lanes, every access to the [field][B] store a coalesced wave transaction.
//   lmpc_ekf_predict_kernel      x_p = f_d(x, u, k = 0, dt), P_p = F P F' + Q   (ekf_state_estimator.cpp:142-146)
//   lmpc_ekf_correct_kernel<NZ>  y, S, K, x, P, the NaN / Inf fallback, check_cov, the clip   (:155-202, :238-264)
//   lmpc_ekf_seed_kernel         per-car or broadcast start of x and P
// The first two are thin wrappers: what a car does in either step is the text of lmpc_ekf_steps.hip.h (lmpc_ekf_predict_car,
// lmpc_ekf_correct_car<NZ>), which lmpc_estimated_loop_kernel.hip chains with the plant, the sensors and the projection.
#include <hip/hip_runtime.h>

#include "lmpc_device.h"
#include "lmpc_dynamics.hip.h"
#include "lmpc_ekf.h"
#include "lmpc_ekf_steps.hip.h"

namespace {

// `final`: the update has no observation -- clip, write the caller's arrays and the flags here.  Otherwise x_p goes to the store
// unclipped and lmpc_ekf_correct_kernel finishes the update.
__global__ __launch_bounds__(256) void lmpc_ekf_predict_kernel(lmpc_vehicle veh, lmpc_ekf_consts cst, lmpc_ekf_store st, double dt, int final,
                                                               lmpc_ekf_out out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= st.B) return;
  const bool ok = lmpc_ekf_predict_car(veh, cst, st, b, dt, final, out);
  if (final && out.flags) out.flags[b] = ok ? 0 : LMPC_EKF_NOT_FINITE;
}

// The correction by an observation of NZ selected rows, z [NZ][B], R [NZ][NZ][B].
template <int NZ>
__global__ __launch_bounds__(256) void lmpc_ekf_correct_kernel(lmpc_ekf_consts cst, lmpc_ekf_store st, lmpc_ekf_obs ob, const double* __restrict__ z,
                                                               const double* __restrict__ R, lmpc_ekf_out out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const size_t B = (size_t)st.B;
  if (b >= st.B) return;
  double zv[NZ], xe[6];
#pragma unroll
  for (int a = 0; a < NZ; ++a) zv[a] = z[a * B + b];
  const int flags = lmpc_ekf_correct_car<NZ>(cst, st, ob, b, zv, R, out, xe);
  if (out.flags) out.flags[b] = flags;
}

__global__ __launch_bounds__(256) void lmpc_ekf_seed_kernel(lmpc_ekf_store st, lmpc_ekf_seed seed, const double* __restrict__ xs,
                                                            const double* __restrict__ Ps) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const size_t B = (size_t)st.B;
  if (b >= st.B) return;
#pragma unroll
  for (int r = 0; r < 6; ++r) st.x[r * B + b] = xs ? xs[r * B + b] : seed.x0[r];
#pragma unroll
  for (int e = 0; e < 36; ++e) st.P[e * B + b] = Ps ? Ps[e * B + b] : seed.P0[e];
}

template <int NZ>
void launch_correct(hipStream_t stream, dim3 grid, const lmpc_ekf_store& st, const lmpc_ekf_consts& cst, const lmpc_ekf_obs& ob, const double* z,
                    const double* R, const lmpc_ekf_out& out) {
  hipLaunchKernelGGL((lmpc_ekf_correct_kernel<NZ>), grid, dim3(256), 0, stream, cst, st, ob, z, R, out);
}

}  // namespace

hipError_t lmpc_ekf_launch(hipStream_t stream, const lmpc_ekf_store& st, const lmpc_vehicle& veh, const lmpc_ekf_consts& cst,
                           const lmpc_ekf_obs* obs, double dt, const double* z, const double* R, const lmpc_ekf_out& out) {
  const dim3 grid((st.B + 255) / 256);
  hipLaunchKernelGGL(lmpc_ekf_predict_kernel, grid, dim3(256), 0, stream, veh, cst, st, dt, obs ? 0 : 1, out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !obs) return e;
  switch (obs->nz) {
    case 1: launch_correct<1>(stream, grid, st, cst, *obs, z, R, out); break;
    case 2: launch_correct<2>(stream, grid, st, cst, *obs, z, R, out); break;
    case 3: launch_correct<3>(stream, grid, st, cst, *obs, z, R, out); break;
    case 4: launch_correct<4>(stream, grid, st, cst, *obs, z, R, out); break;
    case 5: launch_correct<5>(stream, grid, st, cst, *obs, z, R, out); break;
    case 6: launch_correct<6>(stream, grid, st, cst, *obs, z, R, out); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t lmpc_ekf_seed_launch(hipStream_t stream, const lmpc_ekf_store& st, const lmpc_ekf_seed& seed, const double* xs, const double* Ps) {
  hipLaunchKernelGGL(lmpc_ekf_seed_kernel, dim3((st.B + 255) / 256), dim3(256), 0, stream, st, seed, xs, Ps);
  return hipGetLastError();
}
