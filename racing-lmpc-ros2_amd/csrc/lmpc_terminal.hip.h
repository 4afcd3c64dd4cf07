// lmpc_terminal.hip.h -- the safe-set terminal block of the learning problem (always carried in fp64).
// Holds: the TL_* offsets of the terminal region, MA_MAX / TAU_REL, spd_inv6, simplex_bl*, cinv_apply, term_factor_u, term_solve_u.
// Needs: lmpc_wave.hip.h (fences, reductions, frcp / frsqrt).  Included by lmpc_solve_kernel.hip (all three translation units;
// only the learning instantiations, KS > 0, use it).
#ifndef LMPC_TERMINAL_HIP_H_
#define LMPC_TERMINAL_HIP_H_

#include "lmpc_wave.hip.h"

// LMPC extension of the tail (only allocated when learning): terminal-block quantities (see term_factor_u)
// (offsets in `treal` cells from the start of the terminal region, which follows the real-typed records and tail)
#define TL_PT 0      // PT[6][6]: terminal cost-to-go contributed by the safe-set block
#define TL_TG 36     // terminal gradient contribution  E eps + pT
#define TL_EPS 42    // eps = (x_T - ss0) - (SS - ss0 1') lambda
#define TL_FB 48     // F_B^-1 [6][6], F_B = E^-1 + U_B Th_B^-1 U_B' (the points eliminated through 1/theta)
#define TL_WA 84     // W_A = F_B^-1 U_A, column a at +6a
#define TL_UA 120    // u of the explicit points, point a at +6a
#define TL_LC 156    // C_A^-1 [6][6] (full, symmetric), C_A = Theta_A + U_A'F_B^-1 U_A; C_A itself while it is being formed
#define TL_X1 192    // C_A^-1 (1_A - W_A'a_B)
#define TL_G 198     // g = E U M^-1 1
#define TL_AB 204    // a_B = U_B Th_B^-1 1
#define TL_RA 210    // right-hand side of the explicit points (written by their owner lanes)
#define TL_THA 216   // theta of the explicit points
#define TL_XA 222    // their step d lambda_A (read back by the owner lanes)
#define TL_S11 228   // s11 = 1'M^-1 1
#define TL_E 230     // E = 2 convex_hull_slack (exact, whatever `real` is)
#define TL_Z 236     // Z = C_A^-1 W_A' [6][6] (a product of term_factor_u)
#define TL_UL 272    // the (centred) safe-set points, point-major [S][6]
// Explicit points at most (the smallest theta below tau).  Four until round 5 ("supports of 1-3 points are what occurs"): with a
// FIVE-lap safe set the optimum blends one point per lap, a support of five, on ~0.1 % of the bench distribution at N = 27 .. 29
// and on most problems at N <= 5 (tests/dispatch_sweep.py found them).  The fifth point then went through 1 / theta with theta ->
// 1e-12: cond(F_B) 1e12, Newton steps with a stationarity residual of O(1), and an answer 1e-2 from the optimum reported OPTIMAL --
// by the kernel and its twin alike, so kernel-against-twin tests could not see it; the dense oracle did.  Six is what the terminal
// block can hold (C_A = Theta_A + U_A'F_B^-1 U_A has rank <= 6 as Theta_A -> 0) and what its LDS cells were laid out for.
#define MA_MAX 6
#define TAU_REL 1e-5   // tau = TAU_REL * max_j u_j'E u_j: cond(F_B) <= ~1e5 whatever the iteration does

// Inverse of a symmetric positive definite 6x6 (row-major, full storage) by Cholesky; every index is
// a compile-time constant after unrolling, so the factor lives in registers.  Executed redundantly by
// all lanes on wave-uniform data.
template <typename real>
__device__ __forceinline__ void spd_inv6(const real (&F)[36], real (&Fi)[36]) {
  real Lc[36];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    real d = F[j * 6 + j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= Lc[j * 6 + k] * Lc[j * 6 + k];
    d = sqrt(d);
    const real id = 1.0 / d;
    Lc[j * 6 + j] = id;  // store the reciprocal of the pivot
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      real t = F[i * 6 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= Lc[i * 6 + k] * Lc[j * 6 + k];
      Lc[i * 6 + j] = t * id;
    }
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    real y[6], x[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      real t = (i == c) ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < i; ++k) t -= Lc[i * 6 + k] * y[k];
      y[i] = t * Lc[i * 6 + i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
      real t = y[i];
#pragma unroll
      for (int k = i + 1; k < 6; ++k) t -= Lc[k * 6 + i] * x[k];
      x[i] = t * Lc[i * 6 + i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) Fi[i * 6 + c] = x[i];
  }
}

// LMPC simplex row j: gradient of the (eps-eliminated) terminal cost wrt lambda_j including the row's
// barrier coefficient, bl_j = ss_j - cf_j - u_j'E eps; also returns 1/theta_j.
// (ee = E eps of this iteration, wave-uniform)
template <typename real>
__device__ __forceinline__ real simplex_bl(real lm, real t, real l, real pprod, real ssj, const real (&u)[6],
                                             real smu, real pm, const real (&ee)[6], real& itf) {
  const real it_ = frcp(t);
  const real th = l * it_;
  itf = frcp(th);
  const real cf = th * (-lm + t) + (smu - pm * pprod) * it_;
  real ue = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) ue += u[k] * ee[k];
  return ssj - cf - ue;
}

// The same row in a polish round: barrier coefficient y + theta (-lambda_j) if the row lambda_j >= 0 is held (weight theta),
// none if lambda_j is free (it is then one of the explicit unknowns: 1/theta is not used).
template <typename real>
__device__ __forceinline__ real simplex_bl_polish(real lm, real y, bool held, real ssj, const real (&u)[6], const real (&ee)[6],
                                                    real& itf) {
  itf = held ? real(1.0 / POLISH_THETA_L) : real(0);
  const real cf = held ? y - real(POLISH_THETA_L) * lm : real(0);
  real ue = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) ue += u[k] * ee[k];
  return ssj - cf - ue;
}

// ---- terminal block: two-level elimination of the simplex weights (oracle/c/lmpc_oracle.c documents the derivation) ----
// Points with theta >= tau (B) are eliminated through 1/theta and enter as wave sums (T_B, a_B, s_B); the few points
// whose lambda stays positive have theta -> 0 and are kept as explicit unknowns (A, at most MA_MAX): nothing is ever
// divided by a small theta, and cond(F_B) stays below ~1/TAU_REL.  Everything here is wave-uniform arithmetic on values
// every lane holds; results go to the LDS tail (lane 0 writes), the per-right-hand-side solves read them back as
// broadcast reads.  Unused explicit slots (a >= m) hold u = 0, theta = 1, so they drop out without a branch.
// x <- C_A^-1 x.  Lane `la` (< MA_MAX) brings component la of x in `v` and holds row la of C_A^-1 in `ci`; every lane gets all
// of the result.  (Until round 5 every lane carried the whole Cholesky factor and ran both substitutions itself: with six
// explicit points that is 21 live values and two dependent chains of 21 operations per right-hand side.)
template <typename real>
__device__ __forceinline__ void cinv_apply(const real (&ci)[MA_MAX], real v, real (&x)[MA_MAX]) {
  real s = 0.0;
#pragma unroll
  for (int b = 0; b < MA_MAX; ++b) s += ci[b] * lane_bcast(v, b);
#pragma unroll
  for (int a = 0; a < MA_MAX; ++a) x[a] = lane_bcast(s, a);
}

// F = E^-1 + T_B (full 6x6), a_B, s_B, m explicit points (their u, theta already in T[TL_UA], T[TL_THA]).
// Writes F_B^-1, W_A, C_A^-1, x1, g, a_B, s11 and PT = F^-1 + g g'/s11 to the LDS tail.
// The two Cholesky factors are wave-uniform arithmetic in registers (every lane holds the sums they start from); the
// products in between run one OUTPUT per lane -- a column of F_B^-1 or C_A^-1, an element of W_A, C_A, Z, PT -- on operands
// fetched from LDS in one batch per stage, results to LDS (each cell has one writer), a fence, next stage.  An earlier form
// computed everything in every lane with lane 0 storing: ~300 dependent LDS round trips per call, 26 k cycles per
// iteration at one wave per SIMD.
template <typename real>
__device__ __forceinline__ void term_factor_u(real* T, int lane, const real (&F)[36], const real (&aB)[6], real sB, int m) {
  {  // F_B^-1 by Cholesky: lane c < 6 solves for column c
    real Lf[36];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      real d = F[j * 6 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) d -= Lf[j * 6 + k] * Lf[j * 6 + k];
      const real id = frsqrt(d);
      Lf[j * 6 + j] = id;  // reciprocal pivot
#pragma unroll
      for (int i = j + 1; i < 6; ++i) {
        real t = F[i * 6 + j];
#pragma unroll
        for (int k = 0; k < j; ++k) t -= Lf[i * 6 + k] * Lf[j * 6 + k];
        Lf[i * 6 + j] = t * id;
      }
    }
    const int c = lane < 6 ? lane : 0;
    real y[6], x[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      real t = (i == c) ? real(1) : real(0);
#pragma unroll
      for (int k = 0; k < i; ++k) t -= Lf[i * 6 + k] * y[k];
      y[i] = t * Lf[i * 6 + i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
      real t = y[i];
#pragma unroll
      for (int k = i + 1; k < 6; ++k) t -= Lf[k * 6 + i] * x[k];
      x[i] = t * Lf[i * 6 + i];
    }
    if (lane < 6) {
#pragma unroll
      for (int i = 0; i < 6; ++i) T[TL_FB + i * 6 + lane] = x[i];
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) T[TL_AB + k] = aB[k];
    }
  }
  wave_fence();
  {  // W[a][r] = sum_c F_B^-1[r][c] u_a[c]: lane 6a + r
    const int l = lane < 6 * MA_MAX ? lane : 0, a = (l * 43) >> 8, r = l - 6 * a;
    real fb[6], ua[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      fb[c] = T[TL_FB + r * 6 + c];
      ua[c] = T[TL_UA + a * 6 + c];
    }
    real v = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) v += fb[c] * ua[c];
    if (lane < 6 * MA_MAX) T[TL_WA + lane] = v;
  }
  wave_fence();
  {  // C_A = Theta_A + U_A'W_A, staged through the cells of its inverse: lane 6a + b
    static_assert(MA_MAX == 6, "lane mapping of C_A, stride of its cells");
    const int l = lane < 36 ? lane : 0, a = (l * 43) >> 8, bq = l - 6 * a;
    real ua[6], wb[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      ua[r] = T[TL_UA + a * 6 + r];
      wb[r] = T[TL_WA + bq * 6 + r];
    }
    real v = (a == bq) ? T[TL_THA + a] : real(0);
#pragma unroll
    for (int r = 0; r < 6; ++r) v += ua[r] * wb[r];
    if (lane < 36) T[TL_LC + a * 6 + bq] = v;
  }
  wave_fence();
  {  // C_A^-1 by Cholesky, like F_B^-1: the factor in registers (wave-uniform), lane c < MA_MAX solves for column c.  A jitter for
     // identical points (the padding repeats the last point of the set: C_A is then singular as theta -> 0).  An unused slot
     // (a >= m) has u = 0, theta = 1: its row and column of C_A are those of the identity, and so are its inverse's.
    real Lc[36];
    real jit = 0.0;
#pragma unroll
    for (int a = 0; a < MA_MAX; ++a) {
#pragma unroll
      for (int bq = 0; bq <= a; ++bq) Lc[a * 6 + bq] = T[TL_LC + a * 6 + bq];
      jit += Lc[a * 6 + a];
    }
    jit *= real(sizeof(real) == 4 ? 1e-6 : 1e-13);
#pragma unroll
    for (int a = 0; a < MA_MAX; ++a) {
#pragma unroll
      for (int bq = 0; bq <= a; ++bq) {
        real v = Lc[a * 6 + bq] + (a == bq ? jit : real(0));
#pragma unroll
        for (int k = 0; k < bq; ++k) v -= Lc[a * 6 + k] * Lc[bq * 6 + k];
        Lc[a * 6 + bq] = (a == bq) ? frsqrt(v) : v * Lc[bq * 6 + bq];
      }
    }
    const int c = lane < MA_MAX ? lane : 0;
    real y[MA_MAX], x[MA_MAX];
#pragma unroll
    for (int i = 0; i < MA_MAX; ++i) {
      real t = (i == c) ? real(1) : real(0);
#pragma unroll
      for (int k = 0; k < i; ++k) t -= Lc[i * 6 + k] * y[k];
      y[i] = t * Lc[i * 6 + i];
    }
#pragma unroll
    for (int i = MA_MAX - 1; i >= 0; --i) {
      real t = y[i];
#pragma unroll
      for (int k = i + 1; k < MA_MAX; ++k) t -= Lc[k * 6 + i] * x[k];
      x[i] = t * Lc[i * 6 + i];
    }
    wave_fence();  // (every lane has read C_A before its cells take the inverse)
    if (lane < MA_MAX) {
#pragma unroll
      for (int i = 0; i < MA_MAX; ++i) T[TL_LC + i * 6 + lane] = x[i];
    }
  }
  wave_fence();
  // x1 = C_A^-1 (1_A - W_A'a_B), z1 = a_B + U_A x1, g = F_B^-1 z1, s11 = 1_A'x1 + s_B - a_B'g: a row per lane, the
  // vectors from one product to the next through v_readlane
  real s11 = sB;
  {
    const int la = lane < MA_MAX ? lane : 0, lr = lane < 6 ? lane : 0;
    real wa[6], fb[6], ua[MA_MAX], ci[MA_MAX];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      wa[r] = T[TL_WA + la * 6 + r];
      fb[r] = T[TL_FB + lr * 6 + r];
    }
#pragma unroll
    for (int a = 0; a < MA_MAX; ++a) {
      ua[a] = T[TL_UA + a * 6 + lr];
      ci[a] = T[TL_LC + la * 6 + a];
    }
    real x1[MA_MAX], g[6];
    {
      real v = la < m ? real(1) : real(0);
#pragma unroll
      for (int r = 0; r < 6; ++r) v -= wa[r] * aB[r];
      cinv_apply(ci, v, x1);
    }
    real z1u[6];
    {
      real z = aB[0];
#pragma unroll
      for (int k = 1; k < 6; ++k) z = (lr == k) ? aB[k] : z;
#pragma unroll
      for (int a = 0; a < MA_MAX; ++a) {
        z += ua[a] * x1[a];
        s11 += a < m ? x1[a] : real(0);
      }
#pragma unroll
      for (int c = 0; c < 6; ++c) z1u[c] = lane_bcast(z, c);
    }
    {
      real v = 0.0;
#pragma unroll
      for (int c = 0; c < 6; ++c) v += fb[c] * z1u[c];
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        g[r] = lane_bcast(v, r);
        s11 -= aB[r] * g[r];
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) T[TL_G + k] = g[k];
#pragma unroll
      for (int a = 0; a < MA_MAX; ++a) T[TL_X1 + a] = x1[a];
      T[TL_S11] = s11;
    }
  }
  {  // Z = C_A^-1 W_A': lane 6a + c
    const int l = lane < 36 ? lane : 0, a = (l * 43) >> 8, c = l - 6 * a;
    real v = 0.0;
#pragma unroll
    for (int bq = 0; bq < MA_MAX; ++bq) v += T[TL_LC + a * 6 + bq] * T[TL_WA + bq * 6 + c];
    if (lane < 36) T[TL_Z + a * 6 + c] = v;
  }
  wave_fence();
  {  // PT = F_B^-1 - W_A C_A^-1 W_A' + g g'/s11: lane 6r + c
    const real is11 = frcp(s11);
    const int l = lane < 36 ? lane : 0, r = (l * 43) >> 8, c = l - 6 * r;
    real v = T[TL_FB + r * 6 + c] + T[TL_G + r] * T[TL_G + c] * is11;
#pragma unroll
    for (int a = 0; a < MA_MAX; ++a) v -= T[TL_WA + a * 6 + r] * T[TL_Z + a * 6 + c];
    if (lane < 36) T[TL_PT + lane] = v;
  }
  wave_fence();
}

// One right-hand side: beta = U_B Th_B^-1 r_B, sig = 1'Th_B^-1 r_B (wave sums over B), r_A in T[TL_RA], simplex
// residual r1.  Returns h = E U dlambda and nu; writes the explicit points' step to T[TL_XA] (lane 0).
// The operands (rows of W_A, U_A, F_B^-1, C_A^-1, a_B, g) do not depend on the right-hand side: every lane
// fetches the row it works on in ONE batch of LDS reads, the four short products run one output per lane, and what the
// next product needs of the previous one travels through v_readlane (scalar registers), not through LDS -- at one wave
// per SIMD every dependent LDS round trip is ~100 idle cycles, and the all-lanes-compute-everything form of this
// routine had ~100 of them.
template <typename real>
__device__ __forceinline__ void term_solve_u(real* T, int lane, int m, const real (&beta)[6], real sig, real r1, real (&h)[6],
                                             real& nu) {
  const int la = lane < MA_MAX ? lane : 0, lr = lane < 6 ? lane : 0;
  real wa[6], fb[6], ua[MA_MAX], ci[MA_MAX], ab[6], gg[6], x1[MA_MAX];
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    wa[r] = T[TL_WA + la * 6 + r];
    fb[r] = T[TL_FB + lr * 6 + r];
    ab[r] = T[TL_AB + r];
    gg[r] = T[TL_G + r];
  }
  const real ra = T[TL_RA + la], s11 = T[TL_S11];
#pragma unroll
  for (int a = 0; a < MA_MAX; ++a) {
    ua[a] = T[TL_UA + a * 6 + lr];
    x1[a] = T[TL_X1 + a];
    ci[a] = T[TL_LC + la * 6 + a];
  }
  real xa[MA_MAX];
  {
    real v = ra;
#pragma unroll
    for (int r = 0; r < 6; ++r) v -= wa[r] * beta[r];
    cinv_apply(ci, v, xa);
  }
  real num = sig - r1;
  real zu[6];
  {
    real z = beta[0];
#pragma unroll
    for (int k = 1; k < 6; ++k) z = (lr == k) ? beta[k] : z;
#pragma unroll
    for (int a = 0; a < MA_MAX; ++a) {
      z += ua[a] * xa[a];
      num += a < m ? xa[a] : real(0);
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) zu[c] = lane_bcast(z, c);
  }
  {
    real v = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) v += fb[c] * zu[c];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      h[r] = lane_bcast(v, r);
      num -= ab[r] * h[r];
    }
  }
  nu = num * frcp(s11);
#pragma unroll
  for (int r = 0; r < 6; ++r) h[r] = h[r] - nu * gg[r];
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < MA_MAX; ++a) T[TL_XA + a] = xa[a] - nu * x1[a];
  }
  wave_fence();
}

#endif
