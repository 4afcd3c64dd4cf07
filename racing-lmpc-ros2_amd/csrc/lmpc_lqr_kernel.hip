// lmpc_lqr_kernel.hip -- gfx950 kernels of the batched time-varying LQR (csrc/lmpc_lqr.h).  Eight lanes per problem, one matrix
// row per lane, so eight problems share a wavefront; a row of an 8-wide matrix is 8 doubles of a lane, and a product C = X Y takes
// row j of Y from lane j of the group (group_bcast).  Everything stays in registers under compile-time indices; no LDS.
//   lmpc_lqr_discretize_kernel   per (car, stage): (Ac, Bc) at (X_ref[:,k], U_ref[:,k]) with k = 0, [A | B] = top of expm(M dt)
//   lmpc_lqr_recursion_kernel    per car: K_k and P backwards from Qf, then the RK4 rollout under u = U_ref - K (x - X_ref)
// Every loop count is a constant or N: the squaring count is clamped to LMPC_LQR_SQUARINGS_MAX and a NaN norm takes the clamp, so
// no input lengthens a loop.  A group never reads another group's lanes, so one car's NaN stays in its own group.
#include <hip/hip_runtime.h>

#include <utility>

#include "lmpc_device.h"
#include "lmpc_dynamics.hip.h"
#include "lmpc_lqr.h"
#include "lmpc_wave.hip.h"

namespace {

__device__ __forceinline__ bool lqr_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }

// lane J of the group of 8 to the whole group
template <int J>
__device__ __forceinline__ double lqr_bcast(double v) { return group_bcast<0x18 | (J << 5)>(v); }

template <int J>
__device__ __forceinline__ void lqr_bcast_row(const double (&v)[8], double (&o)[8]) {
#pragma unroll
  for (int c = 0; c < 8; ++c) o[c] = lqr_bcast<J>(v[c]);
}
// rows 0 .. 5 of a matrix whose row r is lane r's v
template <int... J>
__device__ __forceinline__ void lqr_rows(const double (&v)[8], double (&o)[6][8], std::integer_sequence<int, J...>) {
  (lqr_bcast_row<J>(v, o[J]), ...);
}
__device__ __forceinline__ void lqr_rows(const double (&v)[8], double (&o)[6][8]) { lqr_rows(v, o, std::make_integer_sequence<int, 6>{}); }

// the group's total in every lane of the group, the same bits in each (every step adds the same two numbers on both sides)
__device__ __forceinline__ double lqr_group_sum(double v) {
  v = v + pair_exchange<0>(v);
  v = v + pair_exchange<1>(v);
  return v + pair_exchange<2>(v);
}
// max that keeps a NaN from either side (fmax drops it)
__device__ __forceinline__ double lqr_nanmax(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double lqr_group_nanmax(double v) {
  v = lqr_nanmax(v, pair_exchange<0>(v));
  v = lqr_nanmax(v, pair_exchange<1>(v));
  return lqr_nanmax(v, pair_exchange<2>(v));
}

// element r of v, r a lane number: selects, not an indexed register array
__device__ __forceinline__ double lqr_pick6(const double (&v)[6], int r) {
  return r == 0 ? v[0] : r == 1 ? v[1] : r == 2 ? v[2] : r == 3 ? v[3] : r == 4 ? v[4] : v[5];
}

// utils::rk4_function (utils.cpp:88-108) with k = 0: the class's own integrator, never Euler
__device__ __forceinline__ void lqr_rk4(const lmpc_vehicle& v, const double* x, double u0, double u1, double dt, double* xp) {
  lmpc_uterms ut;
  lmpc_u_terms(v, u0, u1, ut);
  double k1[6], k2[6], k3[6], k4[6], xs[6];
  lmpc_f<false>(v, ut, x, 0.0, k1, nullptr);
#pragma unroll
  for (int r = 0; r < 6; ++r) xs[r] = x[r] + dt / 2.0 * k1[r];
  lmpc_f<false>(v, ut, xs, 0.0, k2, nullptr);
#pragma unroll
  for (int r = 0; r < 6; ++r) xs[r] = x[r] + dt / 2.0 * k2[r];
  lmpc_f<false>(v, ut, xs, 0.0, k3, nullptr);
#pragma unroll
  for (int r = 0; r < 6; ++r) xs[r] = x[r] + dt * k3[r];
  lmpc_f<false>(v, ut, xs, 0.0, k4, nullptr);
#pragma unroll
  for (int r = 0; r < 6; ++r) xp[r] = x[r] + dt / 6 * (k1[r] + 2 * k2[r] + 2 * k3[r] + k4[r]);
}

__global__ __launch_bounds__(256) void lmpc_lqr_discretize_kernel(lmpc_vehicle veh, lmpc_lqr_store st, int B, const double* __restrict__ X_ref,
                                                                  const double* __restrict__ U_ref) {
  const size_t p = (size_t)blockIdx.x * 32 + (threadIdx.x >> 3);  // problem k B + b
  const int r = threadIdx.x & 7;
  const size_t N = (size_t)st.N, Bz = (size_t)B;
  if (p >= Bz * (N - 1)) return;  // whole groups leave
  const size_t k = p / Bz, b = p - k * Bz;
  double x[6], f[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) x[c] = X_ref[((size_t)c * N + k) * Bz + b];
  const double u0 = U_ref[k * Bz + b], u1 = U_ref[((N - 1) + k) * Bz + b];
  lmpc_uterms ut;
  lmpc_u_terms(veh, u0, u1, ut);
  lmpc_fjac J;
  lmpc_f<true>(veh, ut, x, 0.0, f, &J);  // dynamics_jacobian() without k: curvature 0

  // row r of M = [[Ac, Bc], [0, 0]] dt (the sparsity of lmpc_jvp); rows 6 and 7 are zero
  const double z = 0.0;
  const double r0[8] = {z, J.a01, J.a02, J.a03, J.a04, z, z, z};
  const double r1[8] = {z, z, J.a12, J.a13, J.a14, z, z, z};
  const double r2[8] = {z, -J.k * J.a01, -J.k * J.a02, -J.k * J.a03, -J.k * J.a04, 1.0, z, z};
  const double r3[8] = {z, z, z, J.a3[0], J.a3[1], J.a3[2], J.b3[0], J.b3[1]};
  const double r4[8] = {z, z, z, J.a4[0], J.a4[1], J.a4[2], J.b4[0], J.b4[1]};
  const double r5[8] = {z, z, z, J.a5[0], J.a5[1], J.a5[2], J.b5[0], J.b5[1]};
  double m[8], rowsum = 0.0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const double v = r == 0 ? r0[c] : r == 1 ? r1[c] : r == 2 ? r2[c] : r == 3 ? r3[c] : r == 4 ? r4[c] : r == 5 ? r5[c] : z;
    m[c] = v * st.dt;
    rowsum += fabs(m[c]);
  }
  // halvings: the infinity norm down to 1/2, at most LMPC_LQR_SQUARINGS_MAX of them; `!(<=)` counts a NaN as too large
  double nrm = lqr_group_nanmax(rowsum), scale = 1.0;
  int s = 0;
#pragma unroll 1
  for (int i = 0; i < LMPC_LQR_SQUARINGS_MAX; ++i) {
    if (!(nrm <= 0.5)) nrm *= 0.5, scale *= 0.5, ++s;
  }
  const bool poison = !(nrm <= 0.5);
  if (poison) s = 0;

  double rows[6][8], T[8], E[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    T[c] = m[c] * scale;
    E[c] = (r == c ? 1.0 : 0.0) + T[c];
  }
  lqr_rows(T, rows);  // the scaled matrix' six non-zero rows: every term T_j = T_{j-1} Ms / j is then local to the lane
#pragma unroll 1
  for (int j = 2; j <= LMPC_LQR_TAYLOR_DEGREE; ++j) {
    const double inv = 1.0 / (double)j;
    double Tn[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      double a = 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) a += T[i] * rows[i][c];
      Tn[c] = a * inv;
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) T[c] = Tn[c], E[c] += Tn[c];
  }
#pragma unroll 1
  for (int i = 0; i < LMPC_LQR_SQUARINGS_MAX && i < s; ++i) {  // s is the group's: a group squares or waits as one
    lqr_rows(E, rows);
    double En[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      double a = c >= 6 ? E[c] : 0.0;  // rows 6 and 7 of E are [0 I]
#pragma unroll
      for (int j = 0; j < 6; ++j) a += E[j] * rows[j][c];
      En[c] = a;
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) E[c] = En[c];
  }
  if (r < 6) {
#pragma unroll
    for (int c = 0; c < 8; ++c) st.AB[((k * 8 + c) * Bz + b) * 6 + r] = poison ? __builtin_nan("") : E[c];
  }
}

__global__ __launch_bounds__(256) void lmpc_lqr_recursion_kernel(lmpc_vehicle veh, lmpc_lqr_store st, int B, lmpc_lqr_io io) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int bi = t >> 3, r = t & 7;
  if (bi >= B) return;  // whole groups leave
  const size_t b = (size_t)bi, Bz = (size_t)B, N = (size_t)st.N;
  const bool row = r < 6;  // lanes 6 and 7 carry rows 6 and 7 of [A | B]' and nothing else
  const size_t rc = row ? (size_t)r : 0;
  double Q[6], P[6], R[4];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    Q[c] = row ? st.cfg[rc * 6 + c] : 0.0;
    P[c] = row ? st.cfg[40 + rc * 6 + c] : 0.0;  // P = Qf
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) R[c] = st.cfg[36 + c];
  bool ok = true;

#pragma unroll 1
  for (int kk = (int)N - 2; kk >= 0; --kk) {
    const size_t k = (size_t)kk;
    double ab[8], abt[6];  // row r of [A | B] (r < 6), row r of [A | B]' (all eight lanes)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const double v = st.AB[((k * 8 + c) * Bz + b) * 6 + rc];
      ab[c] = row ? v : 0.0;
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) abt[j] = st.AB[((k * 8 + r) * Bz + b) * 6 + j];
    double rows[6][8], W[8], T[8];
    lqr_rows(ab, rows);
#pragma unroll
    for (int c = 0; c < 8; ++c) {  // W = P [A | B]
      double a = 0.0;
#pragma unroll
      for (int j = 0; j < 6; ++j) a += P[j] * rows[j][c];
      W[c] = a;
    }
    lqr_rows(W, rows);
#pragma unroll
    for (int c = 0; c < 8; ++c) {  // T = [A | B]' W: lanes 0 .. 5 hold A'P[A | B], lanes 6 and 7 G = B'P[A | B]
      double a = 0.0;
#pragma unroll
      for (int j = 0; j < 6; ++j) a += abt[j] * rows[j][c];
      T[c] = a;
    }
    double G0[8], G1[8];
    lqr_bcast_row<6>(T, G0);
    lqr_bcast_row<7>(T, G1);
    // K = solve(R + B'PB, B'PA): a general 2 x 2 elimination with row pivoting, in every lane
    const double s00 = R[0] + G0[6], s01 = R[1] + G0[7], s10 = R[2] + G1[6], s11 = R[3] + G1[7];
    const bool sw = fabs(s10) > fabs(s00);
    const double a0 = sw ? s10 : s00, a1 = sw ? s11 : s01, c0 = sw ? s00 : s10, c1 = sw ? s01 : s11;
    const double l = c0 / a0, d = c1 - l * a1;
    double K0[6], K1[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const double g0 = sw ? G1[c] : G0[c], g1 = sw ? G0[c] : G1[c];
      K1[c] = (g1 - l * g0) / d;
      K0[c] = (g0 - a1 * K1[c]) / a0;
    }
    // P <- Q + A'P(A - B K) = Q + (A'PA - A'PB K), not symmetrised
#pragma unroll
    for (int c = 0; c < 6; ++c) P[c] = row ? Q[c] + (T[c] - T[6] * K0[c] - T[7] * K1[c]) : 0.0;
    const double k0 = lqr_pick6(K0, r), k1 = lqr_pick6(K1, r);  // lane c keeps column c of K_k
    if (row) {
      st.K[((k * 2 + 0) * Bz + b) * 6 + rc] = k0;
      st.K[((k * 2 + 1) * Bz + b) * 6 + rc] = k1;
      if (io.K) {
        io.K[((0 * 6 + rc) * (N - 1) + k) * Bz + b] = k0;
        io.K[((1 * 6 + rc) * (N - 1) + k) * Bz + b] = k1;
      }
      ok = ok && lqr_finite(k0) && lqr_finite(k1);
    }
  }
  if (row) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      ok = ok && lqr_finite(P[c]);
      if (io.P0) io.P0[(rc * 6 + c) * Bz + b] = P[c];
    }
  }

  // the rollout: every lane of the group carries the whole state and evaluates f; lane c owns column c of K and component c of x
  double x[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    x[c] = io.x_ic[c * Bz + b];
    ok = ok && lqr_finite(x[c]);
  }
  if (row) io.X_optm[(rc * N) * Bz + b] = lqr_pick6(x, r);
#pragma unroll 1
  for (size_t k = 0; k + 1 < N; ++k) {
    double p0 = 0.0, p1 = 0.0;
    if (row) {
      const double dx = lqr_pick6(x, r) - io.X_ref[(rc * N + k) * Bz + b];  // the yaw difference is not wrapped, as written
      p0 = st.K[((k * 2 + 0) * Bz + b) * 6 + rc] * dx;
      p1 = st.K[((k * 2 + 1) * Bz + b) * 6 + rc] * dx;
    }
    const double u0 = io.U_ref[k * Bz + b] - lqr_group_sum(p0);
    const double u1 = io.U_ref[((N - 1) + k) * Bz + b] - lqr_group_sum(p1);
    double xn[6];
    lqr_rk4(veh, x, u0, u1, st.dt, xn);
    ok = ok && lqr_finite(u0) && lqr_finite(u1);
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      x[c] = xn[c];
      ok = ok && lqr_finite(x[c]);
    }
    if (r < 2) io.U_optm[((size_t)r * (N - 1) + k) * Bz + b] = r == 0 ? u0 : u1;
    if (row) io.X_optm[(rc * N + k + 1) * Bz + b] = lqr_pick6(x, r);
  }
  const unsigned long long bad = __ballot(!ok);
  if (io.flags && r == 0) io.flags[b] = ((bad >> (threadIdx.x & 56)) & 0xffull) ? LMPC_LQR_NOT_FINITE : 0;
}

}  // namespace

hipError_t lmpc_lqr_launch(hipStream_t stream, const lmpc_lqr_store& st, const lmpc_vehicle& veh, int batch, const lmpc_lqr_io& io) {
  const size_t problems = (size_t)batch * (size_t)(st.N - 1);
  hipLaunchKernelGGL(lmpc_lqr_discretize_kernel, dim3((unsigned)((problems + 31) / 32)), dim3(256), 0, stream, veh, st, batch, io.X_ref, io.U_ref);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(lmpc_lqr_recursion_kernel, dim3((unsigned)((batch + 31) / 32)), dim3(256), 0, stream, veh, st, batch, io);
  return hipGetLastError();
}
