// lmpc_solve_w2.hip.h -- TWO wavefronts per problem on one LDS record: the fp64 tracking kernels for N >= 24 (round 6).
// (Included by lmpc_solve_kernel.hip behind everything it uses as it is: that file's stage chains -- riccati_factor, riccati_solve and
//  feedback_rollout, each ONE call here in the form lmpc_chain_form(LEAN, false) of the instantiation --, its lean model stream, and
//  its active-set polish, lmpc_polish with its argument structs: this file has no polish of its own, it describes the team of two
//  waves (Wave2) that runs the one there; the reductions and pins of lmpc_wave.hip.h, the layout and policies of
//  lmpc_solve_layout.hip.h, the limits of lmpc_limits.hip.h.  A translation unit of its own, lmpc_lib_w2.hip: its object compiles
//  in twenty seconds.)
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

template <class OP, int NV>
__device__ __forceinline__ void wg_reduce_n(Wg2& g, double (&v)[NV]) {
  static_assert(NV <= 8, "eight values per exchange");
  wave_reduce_n<OP, NV>(v);  // (wave-uniform)
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
__device__ __forceinline__ double wg_sum(Wg2& g, double x) {
  double v[1] = {x};
  wg_reduce_n<op_sum, 1>(g, v);
  return v[0];
}
__device__ __forceinline__ double wg_max(Wg2& g, double x) {
  double v[1] = {x};
  wg_reduce_n<op_max, 1>(g, v);
  return v[0];
}
__device__ __forceinline__ double wg_min(Wg2& g, double x) {
  double v[1] = {x};
  wg_reduce_n<op_min, 1>(g, v);
  return v[0];
}
__device__ __forceinline__ bool wg_any(Wg2& g, bool p) { return wg_max(g, __ballot(p) != 0 ? 1.0 : 0.0) > 0.5; }

// ---- the active-set polish on two waves: lmpc_polish itself (lmpc_solve_kernel.hip), run by this team ----
// Wave2 is what lmpc_polish asks of a team (the account stands with Wave1, next to the polish): the rows on 128 threads, the stage
// chains on wave 0 with a barrier behind each, the slot tables read through the empty asm, every exchange one wg_reduce_n -- batched
// where the body has two results to agree on at one point ({largest step, not finite} at the end of a multiplier step; the four votes,
// the most negative multiplier as a maximum of its negative, and the worst row in the KKT test) -- whose barrier also publishes the
// LDS writes before it.  KQ is the class's (the one-wave kernel's slots per lane): it decides the layout; the polish itself is
// instantiated with KL = lmpc_w2_slots(KQ) slots per lane, KS = 0, real = io = double.
template <int KQ, bool CHAIN_>
struct Wave2 {
  static constexpr int THREADS = W2_THREADS;
  static constexpr bool CHAIN = CHAIN_, OPAQUE = true;
  static constexpr bool LEAN = lmpc_lean(8, KQ);
  static constexpr ChainForm FORM = lmpc_chain_form(LEAN, false);  // (pinned addresses: not taken here)
  static constexpr bool PRIO = true;
  const int tid, lane;
  Wg2 g;
  double ex[6];  // what the last step_end / kkt exchange agreed on, by PolishSlot
  __device__ __forceinline__ Wave2() : tid(threadIdx.x), lane(tid & 63), g{nullptr, tid >> 6, 0} {}
  __device__ __forceinline__ void attach(double* tail) { g.red = tail + TL_Y; }
  __device__ static __forceinline__ int table(int v) { asm volatile("" : "+v"(v)); return v; }  // (opaque table reads: see lmpc_solve_problem_w2)
  __device__ static __forceinline__ void sync() { wg_sync(); }
  __device__ static __forceinline__ void published() {}
  __device__ static __forceinline__ void after_chain() { wg_sync(); }
  __device__ __forceinline__ double weights_sum(double q, double x) { return q + wg_sum(g, x); }
  __device__ __forceinline__ void sum3(double (&v)[3]) { wg_reduce_n<op_sum, 3>(g, v); }
  __device__ __forceinline__ void step_end(double stepmax, bool bad) {
    double red[2] = {stepmax, bad ? 1.0 : 0.0};
    wg_reduce_n<op_max, 2>(g, red);
    ex[PS_STEP] = red[0];
    ex[PS_NAN] = red[1];
  }
  __device__ __forceinline__ void kkt(bool bad, bool neg, bool weak, bool viol, double ymin, double worst) {
    double vote[6] = {__ballot(bad) != 0 ? 1.0 : 0.0, __ballot(neg) != 0 ? 1.0 : 0.0, __ballot(weak) != 0 ? 1.0 : 0.0,
                      __ballot(viol) != 0 ? 1.0 : 0.0, -ymin, worst};
    wg_reduce_n<op_max, 6>(g, vote);
#pragma unroll
    for (int k = 0; k < 6; ++k) ex[k] = vote[k];
  }
  // (the lane's own value is not looked at: the exchange has the team's)
  __device__ __forceinline__ bool any_of(int slot, bool) const { return ex[slot] > 0.5; }
  __device__ __forceinline__ double min_of(int slot, double) const { return -ex[slot]; }  // (exchanged as a maximum of its negative)
  __device__ __forceinline__ double max_of(int slot, double) const { return ex[slot]; }
  __device__ __forceinline__ double mean(double x, double inv_m) { return wg_sum(g, x) * inv_m; }
  __device__ __forceinline__ bool changed(bool p) { return wg_any(g, p); }
  __device__ __forceinline__ double sum(double x) { return wg_sum(g, x); }
};

// (a call, as in the one-wave fp64 kernels: lmpc_polish_call; what crosses it stays by value)
template <int KQ, int KL, bool CHAIN>
__device__ __attribute__((noinline)) PolishResult<double, 0> lmpc_polish_call_w2(const PolishArgs<double, KL, 0> a) {
  return lmpc_polish<double, KL, 0, double, Wave2<KQ, CHAIN>>(a);
}

// ---- one problem on two waves: lmpc_solve_problem (lmpc_solve_kernel.hip) for real = io = double, KS = 0, cold start ----
template <int KQ, int KL, int SLOT0, bool CHAIN>
__device__ __forceinline__ void lmpc_solve_problem_w2(const lmpc_params& P, const int B, const int b, unsigned char* lds_raw,
                                                      const double* __restrict__ ws_lin, const double* __restrict__ x_ic,
                                                      const double* __restrict__ u_ic, const double* __restrict__ T_ref,
                                                      const double* __restrict__ bl, const double* __restrict__ br,
                                                      const double* __restrict__ vref, double* __restrict__ X_out, double* __restrict__ U_out,
                                                      double* __restrict__ dU_out, int* __restrict__ status_out, int* __restrict__ iters_out,
                                                      double* __restrict__ kkt_out) {
  typedef double real;
  typedef double2 real2;
  typedef ipm_limits<double> lim;
  typedef polish_limits<double> pol;
  real* const lds = reinterpret_cast<real*>(lds_raw);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int N = P.N, NS = N - 1;
  const real inf = real(INFINITY), marg = real(P.marg), qsig = real(P.qsig), tol = lim::tol(P.tol);
  constexpr bool LEAN = lmpc_lean(8, KQ);
  constexpr ChainForm FORM = lmpc_chain_form(LEAN, false);  // of the stage chains (lmpc_solve_layout.hip.h); pinned addresses: not taken here
  Lds<real> L{lds, N, LEAN ? LMPC_LEAN_STAGE_STRIDE : LMPC_STAGE_STRIDE, true};
  real* T = L.tail();
  real* ct = T + TL_CT;
  real* KN0 = L.kn(0);
  Wg2 g{T + TL_Y, wv, 0};
  ModelStream<real> MS{nullptr, nullptr, NS, lane, -1, -1};
  if constexpr (LEAN) {
    MS.ws = ws_lin + (size_t)b * NS * LMPC_LIN_RECORD;
    MS.buf = T + LMPC_TAIL_DOUBLES;
  }
  PT_DECL
  (void)pf;

  // ---------------- load (lmpc_solve_setup.hip.h: one flight of loads over both waves) ----------------
  lmpc_load_problem<real, real, W2_THREADS, KQ, LEAN, false>(
      P, B, b, tid, L, ws_lin, x_ic, u_ic, T_ref, bl, br, vref, real(0));
  wg_sync();
  PT_MARK(0)

  // ---------------- slot ownership: slot j = SLOT0 + lane + 64 q ----------------
  const bool has_sigma = P.has_sigma != 0;
  const bool fuse = has_sigma;  // the predictor's backward sweep inside the factorisation (riccati_factor<.., FUSE>)
  const int KNB = NS * L.stride;
  const int JB = KNB + N * LMPC_KNOT_STRIDE + TL_W;
  const int CTB = KNB + N * LMPC_KNOT_STRIDE + TL_CT;
  int o_val[KL], o_hl[KL], s_gf[KL];
  real s_tu[KL], s_tl[KL], s_lu[KL], s_ll[KL], s_pu[KL], s_pl[KL];
  real m_rows = 0.0;
#pragma unroll
  for (int q = 0; q < KL; ++q) {
    const int j = SLOT0 + lane + 64 * q;  // (wave 0: slots 0 .. 64 KL0 - 1; wave 1: the rest)
    const bool valid = j < NSLOT * N;
    const int i = valid ? j / NSLOT : 0;
    const int sl = valid ? j - i * NSLOT : 0;
    const int kb = valid ? KNB + i * LMPC_KNOT_STRIDE : JB;
    o_val[q] = kb + (sl < SL_EY ? sl : 1);
    o_hl[q] = (valid && sl < SL_EY) ? CTB + CT_HL + 2 * sl : kb + KN_BHL;
    real hi = inf, lo = -inf;
    bool on = false;
    int ca = CT_ZERO, cb = CT_ZERO, pd = 0;
    if (valid) {
      if (sl < SL_EY) {
        hi = ct[CT_HL + 2 * sl];
        lo = ct[CT_HL + 2 * sl + 1];
        if (sl < SL_U) {
          on = i >= 1 && i <= N - 2;
          ca = (i == N - 1 ? CT_QT : CT_QD) + sl;
        } else {
          const bool uslot = sl < SL_V;
          const int k = uslot ? sl - SL_U : sl - SL_V;
          on = uslot ? i >= 1 : i <= N - 2;
          if (on) {
            ca = (uslot ? CT_QU : CT_SV) + 3 * k;
            cb = (uslot ? CT_QU : CT_SV) + 2 * k + 1 - k;
          }
          pd = k == 0 ? 1 : -1;
        }
      } else {
        hi = lds[kb + KN_BHL];  // bl - marg, br + marg of the knot, as the load left them
        lo = lds[kb + KN_BHL + 1];
        on = has_sigma || i >= 1;
      }
    }
    const bool au = on && (hi < inf), al = on && (lo > -inf);
    const bool eys = valid && sl == SL_EY;
    const int fl = (au ? F_UP : 0) | (al ? F_LO : 0) | ((eys && has_sigma) ? F_SIG : 0) | ((valid && sl == 3) ? F_QLIN : 0) |
                   ((valid && sl < SL_EY && (i >= 1 || sl >= SL_V)) ? F_MOVE : 0) | (eys ? F_EY : 0) | ((eys && i >= 1) ? F_SCH : 0);
    s_gf[q] = ca | (cb << 8) | ((pd + 1) << 16) | (fl << 20) | (sl << 27);
    m_rows += (au ? 1.0 : 0.0) + (al ? 1.0 : 0.0);
    s_tu[q] = s_tl[q] = 1.0;
    s_lu[q] = s_ll[q] = 0.0;
    s_pu[q] = s_pl[q] = 0.0;
  }
  // The slot's table integers as the row phases read them: through an empty asm, so that the LDS addresses derived from them are
  // recomputed at each use (a handful of integer instructions) instead of hoisted out of the iteration -- eight addresses per slot --,
  // spilled, and reloaded one s_waitcnt at a time (lmpc_opaque_slots of the one-wave kernels, profiles/r04_row_phases.md; without
  // it this kernel's gradient took 53 k cycles per iteration at N = 60 against 23 k in the one-wave kernel)
  auto ovq = [&](int q) { int v = o_val[q]; asm volatile("" : "+v"(v)); return v; };
  auto ohq = [&](int q) { int v = o_hl[q]; asm volatile("" : "+v"(v)); return v; };
  auto gfq = [&](int q) { int v = s_gf[q]; asm volatile("" : "+v"(v)); return v; };
  auto flags = [&](int q) { return gfq(q) >> 20; };
  auto o_w = [&](int q) { return ovq(q) + ((flags(q) & F_EY) ? KN_EY - 1 : KN_R0); };
  auto o_csig = [&](int q) { return (flags(q) & F_EY) ? ovq(q) + (KN_CSIG - 1) : JB + KN_CSIG; };
  auto bounds = [&](int q) { return *reinterpret_cast<const real2*>(&lds[ohq(q)]); };
  const real inv_m = real(1) / wg_sum(g, m_rows);

  // knot-0 feasibility
  bool feasible = true;
  {
    bool ok = true;
    if (tid < 6) {
      const real v = KN0[tid];
      ok = (v <= ct[CT_HL + 2 * tid]) && (v >= ct[CT_HL + 2 * tid + 1]);
    }
    if (tid == 6 && !has_sigma) {
      const real ey = KN0[1];
      ok = (ey <= bl[b] - marg) && (ey >= br[b] + marg);
    }
    feasible = wg_min(g, ok ? 1.0 : 0.0) > 0.5;
  }
  real sigma = 0.0;
  const real tau = 0.995, mu0 = 0.1, thr_frac = 0.5;
  int status = LMPC_SOLVE_MAX_ITER, it = 0;
  real mu = 0.0, rdmax = 0.0, rd_check = 0.0, last_step = 0.0, hsig = 0.0, ce = 0.0, mu_prev = inf;
  const int max_iter = feasible ? P.max_iter : 0;
  const bool polish_on = P.polish >= 0;
  bool polished = false, pol_early_done = false, reentry = false, pol_noise = false, distress = false, stall_moving = false;
  int pol_rounds = 0;
  auto put_primal = [&]() {
    const size_t xk = P.out_aos ? 1 : (size_t)N * B, xi = P.out_aos ? 6 : (size_t)B, xb = P.out_aos ? (size_t)6 * N : 1;
    const size_t uk = P.out_aos ? 1 : (size_t)NS * B, ui = P.out_aos ? 2 : (size_t)B, ub = P.out_aos ? (size_t)2 * NS : 1;
    for (int e = tid; e < 6 * N; e += W2_THREADS) {
      const int k = e / N, i = e - k * N;
      X_out[k * xk + i * xi + b * xb] = L.kn(i)[k];
    }
    for (int e = tid; e < 2 * NS; e += W2_THREADS) {
      const int k = e / NS, i = e - k * NS;
      U_out[k * uk + i * ui + b * ub] = L.kn(i + 1)[6 + k];
      dU_out[k * uk + i * ui + b * ub] = L.kn(i)[8 + k];
    }
  };
  auto polish_attempt = [&](int max_rounds) -> bool {
    PolishArgs<real, KL, 0> pa;
    pa.max_rounds = max_rounds;
    pa.keep = reinterpret_cast<double*>(P.save) + (size_t)b * (10 * N - 4);
    pa.ws = MS.ws;
    pa.N = N;
    pa.S = 0;
    pa.has_sigma = P.has_sigma;
    pa.have0 = MS.have0;
    pa.have1 = MS.have1;
    pa.pol_rounds = pol_rounds;
    pa.qsig = qsig;
    pa.inv_m = inv_m;
    pa.sigma = sigma;
#pragma unroll
    for (int q = 0; q < KL; ++q) {
      pa.o_val[q] = o_val[q];
      pa.o_hl[q] = o_hl[q];
      pa.s_gf[q] = s_gf[q];
      pa.s_tu[q] = s_tu[q];
      pa.s_tl[q] = s_tl[q];
      pa.s_lu[q] = s_lu[q];
      pa.s_ll[q] = s_ll[q];
    }
    const PolishResult<real, 0> pr = lmpc_polish_call_w2<KQ, KL, CHAIN>(pa);
    g.par = 0;  // (the polish leaves its exchange parity behind; both waves restart from the same one)
    wg_sync();
    pol_rounds = uni(pr.pol_rounds);
#pragma unroll
    for (int q = 0; q < KL; ++q) s_pu[q] = s_pl[q] = 0.0;
    hsig = 0.0;
    ce = 0.0;
    if constexpr (LEAN) {
      MS.have0 = uni(pr.have0);
      MS.have1 = uni(pr.have1);
    }
    const bool accepted = uni(pr.accepted) != 0;
    pol_noise = uni(pr.noise) != 0;
    if (accepted) {
      sigma = uni(pr.sigma);
      mu = uni(pr.mu);
      rdmax = uni(pr.rdmax);
      last_step = uni(pr.last_step);
    }
    return accepted;
  };

  // ---------------- start point: minimiser of the cost over the dynamics alone ----------------
#pragma unroll
  for (int q = 0; q < KL; ++q) {
    lds[o_w(q)] = 0.0;
    lds[o_csig(q)] = 0.0;
  }
  wg_sync();
  if constexpr (CHAIN) {
    riccati_factor<FORM, false, false>(L, MS, lane, (const double*)nullptr);
    feedback_rollout<FORM>(L, MS, lane);
  }
  wg_sync();
  PT_MARK(1)

  it = -1;
  for (;;) {
    int hand_over = 0;
    for (; it <= max_iter; ++it) {
      const bool ipm = it >= 0;
      // ======== gradient (both waves; with the fused factorisation the predictor's runs AHEAD of the factorisation: lmpc_solve_problem) ========
      real sgsum0 = 0.0;
      auto gradient = [&](const int pass, const real smu, const real pm) -> real {
        const bool fused = fuse && ipm;
        real sgsum = 0.0;
        {
          real val[KL], par[KL], ca[KL], cb[KL], ql[KL];
          real2 hl[KL];
#pragma unroll
          for (int q = 0; q < KL; ++q) {
            const int gr = gfq(q), ov = ovq(q);
            val[q] = lds[ov];
            hl[q] = bounds(q);
            par[q] = lds[ov + ((gr >> 16) & 3) - 1];
            ca[q] = lds[CTB + (gr & 0xff)];
            cb[q] = lds[CTB + ((gr >> 8) & 0xff)];
            ql[q] = lds[ov + (KN_QLIN - 3)];
          }
#pragma unroll
          for (int q = 0; q < KL; ++q) {
            const int f = flags(q);
            const real sg = (f & F_SIG) ? sigma : 0.0;
            const real itu = frcp(s_tu[q]), itl = frcp(s_tl[q]);
            real cu = s_lu[q] * itu * (val[q] - sg + s_tu[q] - hl[q].x) + (smu - pm * s_pu[q]) * itu;
            real cd = s_ll[q] * itl * (-val[q] - sg + s_tl[q] + hl[q].y) + (smu - pm * s_pl[q]) * itl;
            cu = (ipm && (f & F_UP)) ? cu : 0.0;
            cd = (ipm && (f & F_LO)) ? cd : 0.0;
            const real gq = ca[q] * val[q] + cb[q] * par[q] + ((f & F_QLIN) ? ql[q] : real(0));
            lds[o_w(q)] = gq + cu - cd;
            if (pass == 0 && !fused) lds[(f & F_EY) ? JB + KN_EY : o_w(q) + 10] = 0.0;
            sgsum += (f & F_SIG) ? (cu + cd) : real(0);
          }
        }
        wg_sync();
        for (int i = tid; i < N; i += W2_THREADS) {
          real* kn = L.kn(i);
          kn[KN_R0 + 1] += kn[KN_EY];
          if (pass == 0 && !fused) kn[KN_R1 + 1] = (i >= 1) ? kn[KN_CSIG] : 0.0;
        }
        wg_sync();
        return sgsum;
      };
      // ======== rows ========
      if (ipm) {
        real musum = 0.0, rdl = 0.0, eysum = 0.0;
        {
          real val[KL];
          real2 hl[KL];
#pragma unroll
          for (int q = 0; q < KL; ++q) {
            val[q] = lds[ovq(q)];
            hl[q] = bounds(q);
          }
#pragma unroll
          for (int q = 0; q < KL; ++q) {
            const int f = flags(q);
            const real sg = (f & F_SIG) ? sigma : 0.0;
            const real thu = s_lu[q] * frcp(s_tu[q]), thd = s_ll[q] * frcp(s_tl[q]);
            musum += s_lu[q] * s_tu[q] + s_ll[q] * s_tl[q];
            rdl = fmax(rdl, (f & F_UP) ? fabs(val[q] - sg + s_tu[q] - hl[q].x) : real(0));
            rdl = fmax(rdl, (f & F_LO) ? fabs(-val[q] - sg + s_tl[q] + hl[q].y) : real(0));
            lds[o_w(q) + (fuse ? ((f & F_EY) ? KN_TEY - KN_EY : KN_R1 - KN_R0) : 0)] = thu + thd;  // (fused factorisation: the weights in the rhs1 cells)
            lds[o_csig(q)] = (f & F_SIG) ? (thd - thu) : 0.0;
            eysum += (f & F_SIG) ? (thu + thd) : real(0);
          }
        }
        {
          real red[2] = {musum, eysum};
          wg_reduce_n<op_sum, 2>(g, red);
          musum = red[0];
          hsig = qsig + red[1];
        }
        rdmax = wg_max(g, rdl);  // (the two barriers above also publish the barrier weights for the factorisation)
        mu = musum * inv_m;
        if (!reentry && it >= 1 && mu >= mu_prev && rdmax <= lim::rd_distress) distress = true;
        mu_prev = mu;
        const bool again_here = reentry;
        reentry = false;
        if (!(mu == mu) || !(rdmax == rdmax)) {
          status = LMPC_SOLVE_INFEASIBLE;
          break;
        }
        if (mu <= tol && rdmax <= lim::rd_ok) {
          status = LMPC_SOLVE_OPTIMAL;
          hand_over = polish_on ? 2 : 0;
          break;
        }
        if (!again_here && it % 5 == 0) {
          if (it >= 10 && rdmax > lim::rd_infeasible && rdmax > real(0.9) * rd_check) {
            status = LMPC_SOLVE_INFEASIBLE;
            break;
          }
          rd_check = rdmax;
        }
        if (it == max_iter) break;
        if (polish_on && !pol_early_done && mu <= real(pol::mu_early) && rdmax <= real(pol::rd_early)) {
          pol_early_done = true;
          hand_over = 1;
          break;
        }
        PT_MARK(2)
        if (fuse) {
          sgsum0 = gradient(0, real(0), real(0));
          PT_MARK(12)
        }
        if constexpr (CHAIN) {
          if (mu <= real(JOSEPH_MU)) {
            if (fuse)
              riccati_factor<FORM, false, true, true>(L, MS, lane, (const double*)nullptr, KN_R1, KN_TEY);
            else
              riccati_factor<FORM, false, true>(L, MS, lane, (const double*)nullptr);
          } else {
            if (fuse)
              riccati_factor<FORM, false, false, true>(L, MS, lane, (const double*)nullptr, KN_R1, KN_TEY);
            else
              riccati_factor<FORM, false, false>(L, MS, lane, (const double*)nullptr);
          }
        }
        wg_sync();
        PT_MARK(3)
      }

      real sigc = 0.0, alpha = 1.0, dsigma = 0.0;
      bool numerics_failed = false, stalled = false;
      real d_val[KL];
      const int npass = ipm ? 2 : 1;
      for (int pass = 0; pass < npass; ++pass) {
        const real smu = (pass == 1) ? sigc * mu : 0.0, pm = (pass == 1) ? 1.0 : 0.0;
        real sgsum = sgsum0;
        if (!(fuse && ipm && pass == 0)) sgsum = gradient(pass, smu, pm);
        PT_MARK(12)
        // ======== Newton step (wave 0) ========
        if constexpr (CHAIN) {
          if (pass == 0 && ipm && has_sigma) {
            if (fuse)
              riccati_solve<FORM, 2, true>(L, MS, lane, pf);
            else
              riccati_solve<FORM, 2>(L, MS, lane, pf);
          } else
            riccati_solve<FORM, 1>(L, MS, lane, pf);
        }
        wg_sync();
        PT_MARK(4)
        // ======== steps ========
        real dz0[KL], dz1[KL], val[KL];
        real2 hl[KL];
#pragma unroll
        for (int q = 0; q < KL; ++q) {
          dz0[q] = lds[ovq(q) + 10];
          dz1[q] = lds[ovq(q) + 20];
          val[q] = lds[ovq(q)];
          hl[q] = bounds(q);
        }
        if (!ipm) {
#pragma unroll
          for (int q = 0; q < KL; ++q) d_val[q] = dz0[q];
          break;
        }
        if (has_sigma) {
          real red[3] = {0.0, 0.0, sgsum};
          real cs[KL];
#pragma unroll
          for (int q = 0; q < KL; ++q) cs[q] = lds[o_csig(q)];
#pragma unroll
          for (int q = 0; q < KL; ++q) {
            const bool sch = (flags(q) & F_SCH) != 0;
            red[0] += sch ? cs[q] * dz0[q] : real(0);
            red[1] += sch ? cs[q] * dz1[q] : real(0);
          }
          wg_reduce_n<op_sum, 3>(g, red);
          if (pass == 0) ce = red[1];
          const real qsg = qsig * sigma - red[2];
          dsigma = uni(-(qsg + red[0]) / (hsig + ce));
        }
        real dtu[KL], dlu[KL], dtl[KL], dll[KL];
        real rmax = 1.0;
        bool finite_step = true;
#pragma unroll
        for (int q = 0; q < KL; ++q) {
          const int f = flags(q);
          const real dval = dz0[q] + dsigma * dz1[q];
          d_val[q] = dval;
          finite_step = finite_step && (fabs(dval) < inf);
          const real sg = (f & F_SIG) ? sigma : 0.0, dsg = (f & F_SIG) ? dsigma : 0.0;
          const real itu = frcp(s_tu[q]), itl = frcp(s_tl[q]);
          const real a_ = (f & F_UP) ? -(val[q] - sg + s_tu[q] - hl[q].x) - (dval - dsg) : 0.0;
          const real b_ = (f & F_UP) ? -s_lu[q] + (smu - pm * s_pu[q]) * itu - s_lu[q] * itu * a_ : 0.0;
          const real c_ = (f & F_LO) ? -(-val[q] - sg + s_tl[q] + hl[q].y) - (-dval - dsg) : 0.0;
          const real d_ = (f & F_LO) ? -s_ll[q] + (smu - pm * s_pl[q]) * itl - s_ll[q] * itl * c_ : 0.0;
          dtu[q] = a_;
          dlu[q] = b_;
          dtl[q] = c_;
          dll[q] = d_;
          rmax = fmax(rmax, fmax(-a_ * itu, -b_ * frcp(fmax(s_lu[q], lim::tiny))));
          rmax = fmax(rmax, fmax(-c_ * itl, -d_ * frcp(fmax(s_ll[q], lim::tiny))));
        }
        rmax = wg_max(g, finite_step ? rmax : inf);
        if (!(rmax < inf) || !(dsigma == dsigma)) {
          numerics_failed = true;
          break;
        }
        const real amax = real(1) / rmax;
        if (pass == 1) {
          alpha = fmin(real(1), tau * amax);
          if (KQ <= 7 && distress) {  // the wide-neighbourhood rule of the N <= 40 kernels (lmpc_solve_problem; mirrored by the twin)
            for (int trial = 0; trial < NBHD_TRIALS; ++trial) {
              real sl = 0.0, pmin = inf;
#pragma unroll
              for (int q = 0; q < KL; ++q) {
                const int f = flags(q);
                const real pu = (s_tu[q] + alpha * dtu[q]) * (s_lu[q] + alpha * dlu[q]);
                const real pl = (s_tl[q] + alpha * dtl[q]) * (s_ll[q] + alpha * dll[q]);
                sl += pu + pl;
                pmin = fmin(pmin, fmin((f & F_UP) ? pu : inf, (f & F_LO) ? pl : inf));
              }
              pmin = wg_min(g, pmin);
              if (pmin >= real(NBHD_GAMMA) * wg_sum(g, sl) * inv_m) break;
              alpha = alpha * real(0.6);
            }
          }
        }
        real sacc = 0.0;
#pragma unroll
        for (int q = 0; q < KL; ++q) {
          if (pass == 0) {
            sacc += (s_tu[q] + amax * dtu[q]) * (s_lu[q] + amax * dlu[q]) + (s_tl[q] + amax * dtl[q]) * (s_ll[q] + amax * dll[q]);
            s_pu[q] = dtu[q] * dlu[q];
            s_pl[q] = dtl[q] * dll[q];
          } else {
            s_tu[q] += alpha * dtu[q];
            s_lu[q] += alpha * dlu[q];
            s_tl[q] += alpha * dtl[q];
            s_ll[q] += alpha * dll[q];
            sacc += s_tu[q] * s_lu[q] + s_tl[q] * s_ll[q];
          }
        }
        sacc = wg_sum(g, sacc);
        if (pass == 1) {
          if (rdmax <= lim::rd_ok && mu <= real(STALL_MU) && sacc * inv_m >= mu) stalled = true;
        } else {
          const real ratio = (sacc * inv_m) / mu;
          sigc = ratio * ratio * ratio;
        }
      }

      if (numerics_failed) {
        status = (mu <= real(10) * tol && rdmax <= lim::rd_ok) ? LMPC_SOLVE_OPTIMAL : LMPC_SOLVE_MAX_ITER;
        hand_over = (status == LMPC_SOLVE_OPTIMAL && polish_on) ? 2 : 0;
        break;
      }
      if (stalled) {
        // (round 6: a stall is not convergence when the Newton step it declines would still move the iterate -- the point is kept and handed to the
        //  polish as before, but unless the polish verifies it the status is MAX_ITER: oracle/c/lmpc_oracle.c, STALL_STEP, has the problem)
        real cand = 0.0;
#pragma unroll
        for (int q = 0; q < KL; ++q) cand = fmax(cand, (flags(q) & F_MOVE) ? fabs(alpha * d_val[q]) * real(slot_inv_scale((gfq(q) >> 27) & 15)) : real(0));
        stall_moving = wg_max(g, cand) > real(STALL_STEP);
        status = (stall_moving && !polish_on) ? LMPC_SOLVE_MAX_ITER : LMPC_SOLVE_OPTIMAL;
        hand_over = polish_on ? 2 : 0;
        break;
      }
      // ======== primal update ========
      PT_MARK(6)
      real stepmax = 0.0;
#pragma unroll
      for (int q = 0; q < KL; ++q) {
        const bool mv = (flags(q) & F_MOVE) != 0;
        const real dz = mv ? alpha * d_val[q] : 0.0;
        lds[mv ? ovq(q) : JB + q] += dz;
        stepmax = fmax(stepmax, fabs(dz));
      }
      if (ipm) {
        last_step = wg_max(g, stepmax);  // (its barrier also publishes the update)
        if (has_sigma) sigma = sigma + alpha * dsigma;
      } else {
        wg_sync();
        real val[KL];
        real2 hl[KL];
#pragma unroll
        for (int q = 0; q < KL; ++q) {
          val[q] = lds[ovq(q)];
          hl[q] = bounds(q);
        }
#pragma unroll
        for (int q = 0; q < KL; ++q) {
          const int fl = flags(q);
          real range = ((fl & (F_UP | F_LO)) == (F_UP | F_LO)) ? (hl[q].x - hl[q].y) : 1.0;
          if (!(range > real(1e-3))) range = real(1e-3);
          const real thr = thr_frac * range;
          if (fl & F_UP) {
            s_tu[q] = fmax(hl[q].x - val[q], thr);
            s_lu[q] = mu0 / s_tu[q];
          }
          if (fl & F_LO) {
            s_tl[q] = fmax(val[q] - hl[q].y, thr);
            s_ll[q] = mu0 / s_tl[q];
          }
        }
        sigma = 0.0;
      }
    }
    if (hand_over == 0) break;
    wg_sync();
    if (polish_attempt(pol::rounds | (hand_over >= 2 ? POLISH_EXIT : 0))) {
      polished = true;
      status = LMPC_SOLVE_OPTIMAL;
      break;
    }
    if (hand_over == 2) {
      status = LMPC_SOLVE_OPTIMAL;
      if (pol_noise || stall_moving) status = LMPC_SOLVE_MAX_ITER;  // (lmpc_solve_problem: the noise rule, and round 6's stall rule)
      break;
    }
    reentry = true;
  }
  (void)polished;
  PT_MARK(7)
  if (it < 0) it = 0;
  it += pol_rounds;
  if (!feasible) status = LMPC_SOLVE_INFEASIBLE;
  wg_sync();
  put_primal();
  if (CHAIN && lane == 0) {
    status_out[b] = status;
    iters_out[b] = it;
#ifdef LMPC_PHASE_TIMING
    if (kkt_out) {  // (scratch/phase_timing.py: the chain wave's clock)
      for (int k = 0; k < 16; ++k) kkt_out[k * (size_t)B + b] = (double)pf.acc[k];
      kkt_out[16 * (size_t)B + b] = (double)pf.w0;
      kkt_out[17 * (size_t)B + b] = (double)wall_clock64();
      unsigned hwid, xcc;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      kkt_out[18 * (size_t)B + b] = (double)hwid;
      kkt_out[19 * (size_t)B + b] = (double)(xcc & 0xf);
    }
#else
    if (kkt_out) {
      kkt_out[0 * (size_t)B + b] = last_step;
      kkt_out[1 * (size_t)B + b] = rdmax;
      kkt_out[2 * (size_t)B + b] = mu;
      kkt_out[3 * (size_t)B + b] = sigma;
    }
#endif
  }
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
  if ((threadIdx.x >> 6) == 0)  // wave 0 runs the chain phases (by hardware placement instead: no difference, the table above)
    lmpc_solve_problem_w2<KQ, KL, 0, true>(P, B, b, lds_raw, ws_lin, x_ic, u_ic, T_ref, bl, br, vref, X_out, U_out, dU_out, status_out, iters_out,
                                           kkt_out);
  else
    lmpc_solve_problem_w2<KQ, KL, 64 * KL, false>(P, B, b, lds_raw, ws_lin, x_ic, u_ic, T_ref, bl, br, vref, X_out, U_out, dU_out, status_out,
                                                  iters_out, kkt_out);
}

#endif
