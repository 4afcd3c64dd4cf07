// lmpc_solve_w2.hip.h -- TWO wavefronts per problem on one LDS record: the fp64 tracking kernels for N >= 24 (round 6).
// (Included by lmpc_solve_kernel.hip behind everything it uses as it is: that file's interior point, lmpc_solve_problem, and its
//  active-set polish, lmpc_polish with its argument structs.  This file has no iteration and no polish of its own: it holds the
//  workgroup reductions (Wg2, wg_reduce_n), the team of two waves (Wave2) that runs the two bodies there -- the stage chains in the
//  form lmpc_chain_form(LEAN, false) of the class --, the polish's noinline entry and the kernel.  A translation unit of its own,
//  lmpc_lib_w2.hip: its object compiles in twenty seconds.)
//
// Why.  With one wave per problem the slots of the inequality rows are dealt to 64 lanes: 7 per lane at N = 40, 11 at N = 60, 14 at
// N = 80.  A slot is 6 doubles of row state (slacks and multipliers of both sides, the predictor's products) + three table integers
// + the temporaries of whichever row phase is running, so those kernels take the whole register file of a SIMD (512 registers: one
// wave per SIMD) and from N = 41 on spill what does not fit: 992 B of scratch per lane at N = 60, 1792 B at N = 80 -- 28x / 113x the
// algorithmic HBM traffic (profiles/r05_pmc_n60.json).  Here the workgroup is 128 threads: the slots are dealt to 128 lanes (4 / 6 /
// 7 per lane), the kernel is compiled for 256 registers -- two waves per SIMD, i.e. the SAME number of problems per CU as before (LDS
// decides that: 4 at N <= 64, 3 beyond) with twice the waves to run their row phases.
//
// What the second wave does NOT do: the Riccati factorisation and the four vector sweeps of an iteration are one dependent chain
// per problem; they run on ONE wave as in the one-wave kernel while the other waits at the workgroup barrier.  So the chain phases --
// 62 % of the one-wave kernel at N = 60 -- cost what they did (measured, phase clocks of the chain wave: factor 47.0 k cycles per
// iteration against 44.1 k, the four sweeps 118 k against 116 k); what can change is the row phases' share.
//
// Measured (MI355X, 4096 problems, kernel ms; profiles/r06_w2_variants.txt, profiles/r06_fuse_ab.txt):
//                                        N = 24    40     60     80    IAC 40   IAC 80     scratch B / lane (KQ = 7 / 11 / 14)
//   one wave per problem (round 5)        1.63    2.47   5.37   11.44   4.28    13.53      424 /  992 / 1792
//   two waves, five chains per iteration  1.70    2.55   5.37    9.55   4.24    11.38      316 /  740 /  996
//   ... slots dealt unevenly (chain wave 3 / 4 / 4, the other 4 / 7 / 10)
//                                         1.69    2.50   5.67   11.32   4.19    13.27      284 /  896 / 1632
//   ... without the opaque slot tables                   6.23   10.64                      676 / 1276 / 1364
//   ... the chain role by hardware placement (HW_ID) instead of wave 0: no difference (6.48 / 11.10)
//   one wave, fused factorisation         1.56    2.35   5.00    9.70   4.05    11.41      424 / 1008 / 1792
//   two waves, fused (shipped)            1.65    2.47   4.85    8.06   4.15     9.54      316 /  644 /  820
// (fused: the predictor's backward sweep inside the factorisation, riccati_factor<.., FUSE> -- four dependent chains per iteration
//  instead of five.)  The library takes these kernels from N = 41 on -- every lean-layout horizon: -1 .. 4 % up to N = 64, -19 % at N = 65
//  (6.59 -> 5.32 ms: where the one-wave kernel goes from 11 to 14 slots per lane), -17 % at N = 80 -- lmpc_capi.hip: LMPC_W2_AUTO_KQ = 11;
// lmpc_set_waves_per_problem forces either.  Answers: the one-wave kernel's to 1e-11, same statuses, same iteration counts on every
// problem of the six batches.
// Why not more: the chain wave still carries its row state across a Riccati stage that wants ~200 registers of its own, and the
// chains are 75 % of the kernel.  VERDICT r5's targets (N = 60 <= 3.2 ms, N = 80 <= 5.5 ms) need the chain itself shortened further
// (DESIGN.md section 8 has the arithmetic of what was considered).
//
// Exchange between the waves: LDS + s_barrier (wg_sync).  Every wave-wide scalar of the one-wave kernel (mu, the step lengths, the
// Schur sums, the polish's votes) becomes a two-step reduction -- DPP inside each wave, then both partial results through two LDS
// cells, combined in wave order by BOTH waves, so that the two waves hold bit-identical scalars and take every branch together.
#ifndef LMPC_SOLVE_W2_HIP_H_
#define LMPC_SOLVE_W2_HIP_H_

#define W2_THREADS 128
// slots per lane with 128 lanes, dealt evenly to both waves: KQ is the one-wave kernel's (7: N <= 40, 11: N <= 64, 14: N <= 81);
// 128 KL >= 11 N at the class's largest N.  (Measured: dealt unevenly -- the chain wave 3 / 4 / 4, the other 4 / 7 / 10 -- the
// table above.)
constexpr int lmpc_w2_slots(int kq) { return kq <= 7 ? 4 : (kq <= 11 ? 6 : 7); }
static_assert(128 * lmpc_w2_slots(7) >= 11 * 40 && 128 * lmpc_w2_slots(11) >= 11 * 64 && 128 * lmpc_w2_slots(14) >= 11 * 81, "every slot has an owner");

struct Wg2 {
  double* red;  // LDS: [2 parities][2 waves][8 values] -- cells of the factorisation's Y matrix, idle outside the chain phases
  int wv;       // this wave: 0 / 1
  int par;      // parity of the next exchange (alternating buffers: one barrier per reduction)
};
__device__ __forceinline__ void wg_sync() { __syncthreads(); }

// (RID: the wave's half keeps the identity operand of its DPP moves, lmpc_reduce_identity; only lane 63 of it is read either way)
template <class OP, int NV, bool RID>
__device__ __forceinline__ void wg_reduce_n(Wg2& g, double (&v)[NV]) {
  static_assert(NV <= 8, "eight values per exchange");
  wave_reduce_n<OP, NV, RID>(v);  // (wave-uniform)
  double* cell = g.red + g.par * 16;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) cell[g.wv * 8 + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = uni(OP::f(cell[k], cell[8 + k]));  // wave 0's share first, in both waves: the same bits
  g.par ^= 1;
}
template <bool RID>
__device__ __forceinline__ double wg_sum(Wg2& g, double x) {
  double v[1] = {x};
  wg_reduce_n<op_sum, 1, RID>(g, v);
  return v[0];
}
template <bool RID>
__device__ __forceinline__ double wg_max(Wg2& g, double x) {
  double v[1] = {x};
  wg_reduce_n<op_max, 1, RID>(g, v);
  return v[0];
}
template <bool RID>
__device__ __forceinline__ double wg_min(Wg2& g, double x) {
  double v[1] = {x};
  wg_reduce_n<op_min, 1, RID>(g, v);
  return v[0];
}
template <bool RID>
__device__ __forceinline__ bool wg_any(Wg2& g, bool p) { return wg_max<RID>(g, __ballot(p) != 0 ? 1.0 : 0.0) > 0.5; }

// ---- the team of two waves: lmpc_solve_problem and lmpc_polish themselves (lmpc_solve_kernel.hip), run by this team ----
// Wave2 is what the two bodies ask of a team (the account stands with Wave1, next to the polish): the rows on 128 threads, the slots
// dealt from SLOT0 on (wave 0: slots 0 .. 64 KL - 1; wave 1: the rest), the stage chains on wave 0 with a barrier behind each, the slot
// tables read through the empty asm, every exchange one wg_reduce_n -- batched where a body has two results to agree on at one point
// ({musum, eysum} of the rows phase; {largest step, not finite} at the end of a multiplier step; the four votes, the most negative
// multiplier as a maximum of its negative, and the worst row in the KKT test) -- whose barrier also publishes the LDS writes before it.
// KQ is the class's (the one-wave kernel's slots per lane): it decides the layout, the load and the neighbourhood rule; the bodies
// themselves are instantiated with KL = lmpc_w2_slots(KQ) slots per lane, KS = 0, real = io = double, cold start only.
template <int KQ, int KL, bool CHAIN>
__device__ PolishResult<double, 0> lmpc_polish_call_w2(const PolishArgs<double, KL, 0> a);  // (below: it names the team)

template <int KQ, bool CHAIN_>
struct Wave2 {
  static constexpr int THREADS = W2_THREADS, CLASS = KQ, KL = lmpc_w2_slots(KQ), SLOT0 = CHAIN_ ? 0 : 64 * KL;
  static constexpr bool CHAIN = CHAIN_, OPAQUE = true, ROUNDED_CSIG = true;
  static constexpr bool LEAN = lmpc_lean(8, KQ);
  static constexpr ChainForm FORM = lmpc_chain_form(LEAN, false);  // (pinned addresses: not taken here)
  static constexpr bool PRIO = true;
  static constexpr bool LEARN = false;
  static constexpr int ROW_CHUNK = KL, SITES = 0;  // (all slots of a lane in one go)
  static constexpr bool OPAQUE_SLOTS = true, FUSE = lmpc_fuse_bwd(8, KQ, 0);
  static constexpr bool NBHD = KQ <= 7, POLISH_CALL = true;
  static constexpr bool RID = lmpc_reduce_identity(8, KQ, 0, 2);
  const int tid, lane;
  Wg2 g;
  double ex[6];  // what the last step_end / kkt exchange agreed on, by PolishSlot
  __device__ __forceinline__ Wave2() : tid(threadIdx.x), lane(tid & 63), g{nullptr, tid >> 6, 0} {}
  __device__ __forceinline__ void attach(double* tail) { g.red = tail + TL_Y; }
  __device__ static __forceinline__ int table(int v) { asm volatile("" : "+v"(v)); return v; }
  __device__ static __forceinline__ void sync() { wg_sync(); }
  __device__ static __forceinline__ void published() {}
  __device__ static __forceinline__ void after_chain() { wg_sync(); }
  __device__ static __forceinline__ double uniform(double x) { return x; }
  __device__ __forceinline__ double exchanged(double x) { return wg_sum<RID>(g, x); }
  __device__ static __forceinline__ double sum_of(double x) { return x; }
  __device__ static __forceinline__ void publish(bool next) { if (!next) wg_sync(); }
  // (the polish leaves its exchange parity behind; both waves restart from the same one)
  __device__ __forceinline__ void after_polish() { g.par = 0; wg_sync(); }
  template <typename real, typename io>
  static constexpr PolishResult<double, 0> (*polish_call)(const PolishArgs<double, KL, 0>) = &lmpc_polish_call_w2<KQ, KL, CHAIN_>;
  __device__ __forceinline__ void sum2(double (&v)[2]) { wg_reduce_n<op_sum, 2, RID>(g, v); }
  __device__ __forceinline__ double max(double x) { return wg_max<RID>(g, x); }
  __device__ __forceinline__ double min(double x) { return wg_min<RID>(g, x); }
  __device__ __forceinline__ bool all(bool p) { return wg_min<RID>(g, p ? 1.0 : 0.0) > 0.5; }
  __device__ __forceinline__ double weights_sum(double q, double x) { return q + wg_sum<RID>(g, x); }
  __device__ __forceinline__ void sum3(double (&v)[3]) { wg_reduce_n<op_sum, 3, RID>(g, v); }
  __device__ __forceinline__ void step_end(double stepmax, bool bad) {
    double red[2] = {stepmax, bad ? 1.0 : 0.0};
    wg_reduce_n<op_max, 2, RID>(g, red);
    ex[PS_STEP] = red[0];
    ex[PS_NAN] = red[1];
  }
  __device__ __forceinline__ void kkt(bool bad, bool neg, bool weak, bool viol, double ymin, double worst) {
    double vote[6] = {__ballot(bad) != 0 ? 1.0 : 0.0, __ballot(neg) != 0 ? 1.0 : 0.0, __ballot(weak) != 0 ? 1.0 : 0.0,
                      __ballot(viol) != 0 ? 1.0 : 0.0, -ymin, worst};
    wg_reduce_n<op_max, 6, RID>(g, vote);
#pragma unroll
    for (int k = 0; k < 6; ++k) ex[k] = vote[k];
  }
  // (the lane's own value is not looked at: the exchange has the team's)
  __device__ __forceinline__ bool any_of(int slot, bool) const { return ex[slot] > 0.5; }
  __device__ __forceinline__ double min_of(int slot, double) const { return -ex[slot]; }  // (exchanged as a maximum of its negative)
  __device__ __forceinline__ double max_of(int slot, double) const { return ex[slot]; }
  __device__ __forceinline__ double mean(double x, double inv_m) { return wg_sum<RID>(g, x) * inv_m; }
  __device__ __forceinline__ bool changed(bool p) { return wg_any<RID>(g, p); }
  __device__ __forceinline__ double sum(double x) { return wg_sum<RID>(g, x); }
};

// (a call, as in the one-wave fp64 kernels: lmpc_polish_call; what crosses it stays by value)
template <int KQ, int KL, bool CHAIN>
__device__ __attribute__((noinline)) PolishResult<double, 0> lmpc_polish_call_w2(const PolishArgs<double, KL, 0> a) {
  return lmpc_polish<double, KL, 0, double, Wave2<KQ, CHAIN>>(a);
}

// (two waves per SIMD: eight waves = four problems per CU at N <= 64, six = three beyond -- what LDS allows either way)
template <int KQ>
__global__ __launch_bounds__(W2_THREADS, 2) void lmpc_solve_kernel_w2(lmpc_params P, int B, const double* __restrict__ ws_lin,
                                                                       const double* __restrict__ x_ic, const double* __restrict__ u_ic,
                                                                       const double* __restrict__ T_ref, const double* __restrict__ bl,
                                                                       const double* __restrict__ br, const double* __restrict__ vref,
                                                                       double* __restrict__ X_out, double* __restrict__ U_out,
                                                                       double* __restrict__ dU_out, int* __restrict__ status_out,
                                                                       int* __restrict__ iters_out, double* __restrict__ kkt_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  int b = (int)(blockIdx.x & 7) * ((B + 7) >> 3) + (int)(blockIdx.x >> 3);  // (XCD-aware, as lmpc_solve_kernel)
  if (P.launch_order) {
    const int n = P.order_count ? *P.order_count : B;
    b = (int)blockIdx.x < n ? P.launch_order[blockIdx.x] : B;
  }
  if (b >= B) return;
  constexpr int KL = lmpc_w2_slots(KQ);
  // each wave runs lmpc_solve_problem on its half of the slots; wave 0 runs the chain phases (by hardware placement instead: no
  // difference, the table above).  Tracking only: no safe set, no simplex weights.
  if ((threadIdx.x >> 6) == 0)
    lmpc_solve_problem<double, KL, 0, double, false, false, Wave2<KQ, true>>(P, B, b, lds_raw, ws_lin, x_ic, u_ic, T_ref, bl, br, vref, nullptr, nullptr,
                                                                            nullptr, X_out, U_out, dU_out, status_out, iters_out, kkt_out);
  else
    lmpc_solve_problem<double, KL, 0, double, false, false, Wave2<KQ, false>>(P, B, b, lds_raw, ws_lin, x_ic, u_ic, T_ref, bl, br, vref, nullptr, nullptr,
                                                                             nullptr, X_out, U_out, dU_out, status_out, iters_out, kkt_out);
}

#endif
