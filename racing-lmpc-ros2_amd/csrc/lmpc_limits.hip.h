// lmpc_limits.hip.h -- the numbers that decide when the iteration and the polish stop, per precision.
// Holds: STALL_*, NBHD_*, ipm_limits, polish_limits, slot_inv_scale, POLISH_*, WARM_*.  Needs: lmpc_device.h (LMPC_WARM_ROUNDS_MAX).
// Included by lmpc_solve_kernel.hip (all three translation units); oracle/c/lmpc_oracle.c carries the same values.
#ifndef LMPC_LIMITS_HIP_H_
#define LMPC_LIMITS_HIP_H_

#include "lmpc_device.h"

#define STALL_MU 1e-9  // complementarity below which a step that does not lower it ends the solve
#define STALL_STEP 1e-6  // ... and the scaled size of that step above which the stalled iterate, unless the polish verifies it, is MAX_ITER
#define NBHD_GAMMA 1e-2  // once mu has risen: no complementarity product below this fraction of their mean after a step (1e-3
                        // does not stop the cycle the rule is there for; applied to every problem 3e-2 costs 13 % more iterations)
#define NBHD_TRIALS 3   // cuts of the step length by 0.6 at most (two are what the cycling problem needs; bounded so that a point already
                        // outside the neighbourhood cannot freeze the iteration)

// Per-precision constants of the iteration.  fp32: the complementarity floor of a single-precision Riccati
// recursion is ~1e-6 (weights lam/t ~ 1e5 already cancel four digits in P), rows are feasible to ~1e-4.
template <typename real> struct ipm_limits;
template <> struct ipm_limits<double> {
  static __device__ __forceinline__ double tol(double cfg) { return cfg; }
  static constexpr double rd_ok = 1e-9, rd_infeasible = 1e-6, tiny = 1e-300;
  static constexpr double rd_distress = 1e-6;  // a rise of mu counts as distress only in the (nearly) feasible end game
};
template <> struct ipm_limits<float> {
  static __device__ __forceinline__ float tol(double cfg) { return fmaxf((float)cfg, 2e-6f); }
  static constexpr float rd_ok = 1e-4f, rd_infeasible = 1e-2f, tiny = 1e-30f;
  static constexpr float rd_distress = 1e-4f;
};
// Active-set polish (what OSQP's polish = true is to the reference, racing_mpc.cpp:90-95; derivation and measurements in
// oracle/c/lmpc_oracle.c, which runs the same rounds): rows with lam > t are HELD -- weight theta on them, none on the
// others, one stabilised factorisation -- then `steps` multiplier steps on that factor (gradient y + theta * residual on
// the held rows, full Newton step, y <- y + theta * (residual + the row's own increment)), a KKT test (held rows met to
// `feas` with y >= -dual, the others satisfied to `feas`, the last step below step_tol in the reference's scaled units),
// and up to `rounds` repairs of the held set.  Double precision
// tries it once as soon as mu <= mu_early with rows feasible to rd_early -- about two iterations before the interior
// point's own tolerance, and the stabilised factorisations of those iterations are the ones it saves -- and again at
// convergence if refused; single precision polishes at its convergence (mu ~ 2e-6), where it turns "within sqrt(mu) of the
// optimum" into "the optimum to the accuracy of an fp32 solve".
// The acceptance test of the single-precision polish (measured: the tail measurements of profiles/r04_f32_acceptance.md).
// Until round 4: rows to 1e-5, multipliers to -1e-3.  At the batch sizes one GPU runs, that let three answers of 65536 learning
// problems through that the fp32 KKT test verified and the fp64 kernel contradicts: 2.4e-3 away with the regression on (a held
// row's multiplier between -1e-3 and -3e-4), 1.2e-3 and 1.0e-3 without it (a multiplier at -7e-5; a row violated by 3.8e-6).
// With rows to 3e-6 and multipliers to -3e-5 the worst of four 32768-batches is 9.0e-4 (one problem; every other below 2.5e-5)
// and the worst IAC problem 8.5e-5; the fp64 pass gets 4 more problems of 32768 and the solve takes the same time.
template <typename real> struct polish_limits;
template <> struct polish_limits<double> {
  static constexpr bool early = true;
  // Round 5: up to FOUR multiplier steps (the loop stops after the second when that one moved the iterate by <= step_ok), a last
  // step of at most 1e-6 (1e-5 until then) and four rounds (three).  A held set that a repair has extended -- the new rows start
  // from a zero multiplier -- or two boundary rows coupled through sigma converge like 0.1 per step, not at once: the second
  // step was still 1.5e-5 .. 1.7e-4, the attempt was refused, and what stood was the interior point's own answer, 9e-6 (tracking,
  // N = 80) and 2e-5 (learning, N = 60) from the dense optimum; an attempt accepted at 1e-5 with that rate is itself 1e-6 off.
  // Measured on the serial twin against the dense optimum over the bench distributions (scratch/r5/cmp_cache.py): worst 2e-7
  // at every horizon, mean iterations -0.3 %, the slowest problem of the N = 20 batch 18 -> 14 iterations.
  // Round 6: up to SIX steps.  The fused factorisation (riccati_factor<.., FUSE>) changes the last bits of every sweep, and one problem of
  // tests/dispatch_sweep.py's 323 584 (BARC tracking, N = 51) fell on the other side of the limit: its exit attempt's steps go 2.1e-5,
  // 5.9e-6, 1.9e-6, 2.2e-7 on the twin (accepted) and ended just above step_tol in the kernel -- refused, and the interior point's own
  // iterate (mu 5e-12, a degenerate problem: 3.4e-6 from the twin in dU) stood with status OPTIMAL.  A consistent set whose steps are
  // still CONVERGING is not a reason to give the optimum up: two more steps cost two sweeps on the few problems that need them (the
  // loop leaves after any step <= step_ok) and nothing on the others.
  // mu_early stays 1e-8.  1e-7 was measured in round 6 (scratch/r6/twin_mu_early.py on the twin, then on the GPU): mean iterations
  // 8.92 -> 8.63 (BARC N = 20), 9.41 -> 9.17 (N = 40), 12.5 -> 12.2 (learning), every answer still 1e-9 from the dense optimum, the
  // pipelined rate +1.3 % -- and the KERNEL slower: 0.813 -> 0.861 ms (N = 20), 2.35 -> 2.48 (N = 40), 8.11 -> 8.65 (N = 80) per 4096:
  // more early attempts are refused, those problems pay the attempt and a second one, and a launch lasts as long as its slowest waves.
  static constexpr double theta = 1e8, feas = 1e-9, dual = 1e-7, mu_early = 1e-8, rd_early = 1e-6, step_ok = 1e-7, step_tol = 1e-6;
  // dual_l: the same test on the SIMPLEX rows' multipliers, a decade tighter (round 6).  The learning problem is LP-like along blends of
  // nearly exchangeable safe-set points: a wrong vertex whose pinned weights have multipliers of -2e-8 .. -1e-7 passed at -1e-7 and sat
  // 1.4e-3 from the dense optimum in X at an objective gap below 1e-9 (the twin, one problem of the 3.9 M of the large dispatch sweeps:
  // N = 71, 160 points; at -1e-8 it is repaired to the optimum).  No problem of the learning fixtures has a multiplier in between: same
  // iterations, same answers (scratch/r6/twin_mu_early.py with TWIN_MACRO=POLISH_DUAL_L).
  static constexpr double dual_l = 1e-8;
  static constexpr int rounds = 4, steps = 6;
};
template <> struct polish_limits<float> {
  // theta: 1e7 needs the stabilised factor and the fp64 2x2 pivot; with 1e5 chains of held input rows (u_i = u_{i-1} + t v_i,
  // stiffness R_d / t^2 per link) converge like 0.7 per step.  Up to three steps: the third removes what the rounding of the
  // first two has left, and is only taken when the second still moved the iterate by more than step_ok (scaled units).
  static constexpr bool early = false;  // (an early attempt at mu ~ 1e-4 was measured on the serial twin: the iterations it saves are fewer than the rounds it adds)
  static constexpr float theta = 1e7f, feas = 3e-6f, dual = 3e-5f, mu_early = 0.0f, rd_early = 0.0f, step_ok = 3e-6f, step_tol = 1e-4f;
  static constexpr float dual_l = dual;  // (the simplex rows' multipliers: the rows' own limit in single precision)
  static constexpr int rounds = 4, steps = 3;
};
// 1 / scale of the quantity a slot constrains: the reference's scale vectors (racing_mpc.cpp:36-37, hard-coded there for every
// vehicle) -- used only to measure a polish step
__device__ __forceinline__ float slot_inv_scale(int sl) {
  return sl == 0 ? 5e-4f : (sl == 1 || sl == 10) ? 0.1f : sl == 2 ? 10.0f : sl == 3 ? 0.0125f : (sl == 4 || sl == 5) ? 0.5f : (sl == 6 || sl == 8) ? 0.1f : (1.0f / 0.3f);
}
#define POLISH_THETA_L 1e8  // the simplex rows (always fp64)
#define POLISH_STRONG 1e3   // a row with lam >= POLISH_STRONG t is one the interior point holds firmly
#define POLISH_EXIT 256         // flag in PolishArgs::max_rounds: the attempt at the interior point's exit
#define POLISH_EXIT_GAMMA 1e-2  // ... holds a row from lam > 1e-2 t on (early and warm attempts: lam > t)
#define WARM_ROUNDS 2       // repairs a warm start may spend before the cold start takes over
static_assert(polish_limits<double>::rounds == LMPC_WARM_ROUNDS_MAX, "lmpc_set_warm_rounds' upper limit is the polish's");
#define WARM_ACT 1e-9       // a box row of the plan counts as active within this slack (a polished plan sits on its bounds to ~1e-16)
#define WARM_ACT_EY 1e-3    // boundary rows: their bounds move with the shift (the track's half-width over one knot's travel)

#endif
