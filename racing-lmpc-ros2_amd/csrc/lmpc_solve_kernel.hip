// lmpc_solve_kernel.hip -- the batched QP solve of RacingMPC::solve on gfx950 (CDNA4): fp64, and the same source in fp32.
//
// What it replaces: opti_.solve_limited() on the "conic"/OSQP problem built in
//   src/mpc/racing_mpc/src/racing_mpc.cpp:106-201 (constraints), :442-477 (tracking cost),
//   :524-543 (boundary slack); actuator boxes from single_track_planar_model.cpp:113-120,144-151.
//
// Mapping: ONE WAVEFRONT (64 lanes) PER PROBLEM, one wave per workgroup, everything the
// iteration touches resident in LDS (~20 KB at N = 20 -> 8 problems per CU).
//   * Riccati factorisation: the augmented state z = [x; u_prev] has 8 components, so the 8x8
//     cost-to-go matrix is exactly one wave: lane l owns element (r, c) = (l >> 3, l & 7).
//     Matrix products are 6-term dot products whose operands come as LDS row reads (b128; padded /
//     skewed rows keep them bank-conflict free); each lane keeps its own element in a register.
//   * Riccati vector solves: lane (s, r) = (l >> 3, l & 7) computes component r of right-hand
//     side s, so the predictor step and the boundary-slack Schur vector are solved in the same
//     instruction stream (two RHS for the price of one); the running vector makes one LDS trip per
//     stage, the stage's 2-vector is spread with ds_swizzle / v_readlane.
//   * Inequality rows: the 11 two-sided slots of each knot (6 state, 2 input, 2 input-rate,
//     1 track boundary) are dealt round-robin to lanes; slacks and multipliers never leave
//     registers.  The slot owner also owns the primal component the slot constrains: it writes
//     that component's barrier weight and gradient entry and applies its update.
//   * Wave-wide scalars (mu, step length, Schur dot products) are DPP reductions on the VALU and
//     live in SGPRs afterwards.
//   * The whole iteration is a chain of ~120 dependent stage steps: operands that do not depend on
//     the chain are fetched one stage ahead, exchanges through LDS use compiler-only fences (one
//     wave per workgroup: no s_barrier, no wait for the write to retire).
// Too small for MFMA (6..8-wide blocks); the kernel is bound by LDS instruction issue and FP64
// VALU issue, not by HBM.
//
// Algorithm (twin of oracle/c/lmpc_oracle.c, which documents the derivation): Mehrotra
// predictor-corrector interior point; Newton systems by Riccati recursion on (z, v = dU); the
// shared boundary slack sigma (one scalar coupling all knots) by a Schur complement.
//
// This file: the stage chains (Riccati factorisation and feedback rollout: one body each for the indexed, pinned and lean form; the
// vector solve: still a fat and a lean function behind one call), the lean model stream, the active-set polish, lmpc_solve_problem,
// the kernels and the lists of what each translation unit instantiates.  What they are written in -- layouts, policies and the
// description of the chain forms, wave primitives, limits, the safe-set terminal block -- is in the four headers included below (DESIGN.md section 4 has the file map); lmpc_solve_w2.hip.h holds the two-wave kernel.
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "lmpc_device.h"

#include "lmpc_solve_layout.hip.h"   // LDS layouts, Lds / SimplexRows, per-instantiation policies, the forms of a stage chain
#include "lmpc_wave.hip.h"           // fences, broadcasts, reductions, scheduling pins
#include "lmpc_limits.hip.h"         // ipm_limits, polish_limits
#include "lmpc_terminal.hip.h"       // safe-set terminal block

// (the lean layout and its LN_* offsets: lmpc_solve_layout.hip.h)
#include "lmpc_solve_setup.hip.h"    // the load phase of both layouts

// The lean layout's stage model on its way from the linearisation workspace to the two chunk buffers in LDS.
// Streaming discipline of a sweep that walks the stages downwards (factor, backward vector sweep): the chunk it starts in
// is fetched and waited for, the one below it is fetched at once; the stage that reads ahead into the next chunk waits for
// it first and, the chunk just left being dead by then, fetches the one after into its buffer.  Upwards (forward sweep,
// rollout) the mirror image.  One fetch is in flight at a time; a chunk is 8 stages of work ahead of its first use.
// In the chain bodies these steps stand under `if constexpr (SC::lean)`.
template <typename real>
struct ModelStream {
  const real* ws;  // this problem's [N - 1][LN_REC] in the workspace (HBM / L2)
  real* buf;       // LDS: 2 chunks of LN_CHUNK records
  int NS, lane;
  int have0 = -1, have1 = -1;  // the chunk each buffer holds (or is being filled with): a sweep that finds its first chunks
                               // resident -- the forward sweep after a backward one, the factorisation after a forward sweep --
                               // starts without a fetch
  __device__ __forceinline__ void ensure(int ch) {
    if ((ch & 1 ? have1 : have0) != ch) fetch(ch);
  }
  // chunk ch -> buffer (ch & 1), asynchronously: 16 bytes per lane per instruction, the wave's lanes in address order.
  // ONE per-lane address and one LDS base for the whole chunk, the instruction's immediate offset (applied to both sides)
  // steps through it: with an address per instruction the compiler kept seven 64-bit addresses per call site alive,
  // spilled them, and every copy then waited (vmcnt counts the reload and the copies alike) for the one before it.
  __device__ __forceinline__ void fetch(int ch) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (no LDS read of the buffer about to be overwritten is still in flight)
    if (ch & 1) have1 = ch; else have0 = ch;
    const int lo = ch * LN_CHUNK * LN_REC;
    const int n = min(LN_CHUNK * LN_REC, NS * LN_REC - lo);
    real* const dst = buf + (ch & 1) * LN_CHUNK * LN_REC;
    // (the per-lane source address from a lane number the optimiser cannot see through: hoisted out of the sweeps as the loop
    //  invariant it is, the 64-bit address was spilled, and each of the four copies below then waited -- vmcnt(0): for its own
    //  reload AND the copy before it -- four memory round trips in a row per chunk)
    int fl = lane;
    asm volatile("" : "+v"(fl));
    const real* const src = ws + lo + 2 * fl;
    const int e = 2 * fl;
    static_assert(sizeof(real) == 8 && (LN_CHUNK * LN_REC + 127) / 128 == 4, "four 1 KB slices per chunk");
#define LMPC_GLDS(J)                                                                                                   \
  if (e + 128 * J < n)                                                                                                 \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,                               \
                                     (__attribute__((address_space(3))) void*)dst, 16, 1024 * J, 0);
    LMPC_GLDS(0) LMPC_GLDS(1) LMPC_GLDS(2) LMPC_GLDS(3)
#undef LMPC_GLDS
  }
  // every copy issued so far has landed (vmcnt counts them), and no later LDS read moves ahead of this point
#ifdef LMPC_PHASE_TIMING
  mutable long long waited = 0;  // cycles spent in wait() (profiling build: reported as phase 5)
#endif
  __device__ __forceinline__ void wait() const {
#ifdef LMPC_PHASE_TIMING
    const long long t0 = __builtin_readcyclecounter();
#endif
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wave_fence();
#ifdef LMPC_PHASE_TIMING
    waited += __builtin_readcyclecounter() - t0;
#endif
  }
  __device__ __forceinline__ const real* stage(int i) const {  // (i is wave-uniform: keep the slot arithmetic on the scalar unit)
    const int off = __builtin_amdgcn_readfirstlane(((i / LN_CHUNK) & 1) * LN_CHUNK * LN_REC + (i % LN_CHUNK) * LN_REC);
    return buf + off;
  }
};

// true cost Hessian entry on z_i (no barrier terms), racing_mpc.cpp:459-476; terminal knot or a knot 1 <= i <= N-2
template <typename real>
__device__ __forceinline__ real qz_entry(const real* ct, bool terminal, int r, int c) {
  const int rx = r < 6 ? r : 0, ru = r >= 6 ? r - 6 : 0, cu = c >= 6 ? c - 6 : 0;
  const real dx = terminal ? ct[CT_QT + rx] : ct[CT_QD + rx];
  const real uu = ct[CT_QU + ru * 2 + cu];
  return (r < 6 || c < 6) ? ((r == c) ? dx : 0.0) : uu;
}

// ======== the stage chains: factorisation, vector solve, rollout ========
// The factorisation and the LDS-exchange rollout are ONE body each for the three forms an instantiation can take (ChainForm,
// lmpc_solve_layout.hip.h: indexed fat records, fat records on pinned LDS addresses, lean records with the model streamed).  The body
// states the stage arithmetic once; `SC` (StageCells<FORM>) says where the cells of a stage are; CHAIN_GET / CHAIN_PUT reach a cell as
// record(i) + offset or, under CHAIN_PINNED, through an LDS byte address that is set up, pinned and advanced in three blocks under
// `SC::pinned` -- the same cells in the same order --; what the lean form adds (when the chunks of the model are fetched and waited
// for) stands under `SC::lean`.  Every call site passes the form of its instantiation, lmpc_chain_form(LEAN, lmpc_chain_addr(..)).
// The bodies are held to the device code of the separate functions they replace (scratch/isa_diff.py): they avoid lambdas and helper
// functions around their arrays and around control flow on the stage index, which change what the optimiser emits.

// Backward Riccati sweep for the barrier weights currently in the knots' rhs0 region
// (Thz @ +10..17, Thv @ +18,19, boundary weight @ KN_EY).  Leaves K (columns 6,7 of M) and Hinv in
// the stage records.
//
// The sweep is one dependent chain over the knots, so it is written for latency: lane (r, c) keeps its
// own element of P / W in a register, everything that does not depend on the chain (model rows, barrier
// weights) is fetched one stage ahead, and the three exchanges per stage (P, W, Y rows through LDS) are
// the only waits; the 2x2 inverse starts from v_readlane copies of Y_uu while the Y rows are in flight.
//
// JOSEPH selects the stabilised form of the cost-to-go update, P <- Qz + Thz + Phi' P Phi + K' (Sv + Thv) K with
// Phi = Abar - Bbar K: the same matrix in exact arithmetic, but a sum of positive semidefinite products.  The plain form
// Y - G'K subtracts two numbers of the size of the largest barrier weight (1e10 .. 1e13 late in the iteration) to leave
// one of the size of the cost, and the Newton directions lose those digits (the former "mu ~ 1e-11 floor"); here the
// cancellation happens inside Phi, before the multiplication by P.  It costs a second pair of 8x8 products (8-term,
// Phi has no identity block), so the iteration uses it only once mu <= JOSEPH_MU: about two factorisations per solve.
#define JOSEPH_MU 1e-8
//
// FUSE (round 6): the factorisation carries the BACKWARD sweep of the predictor's two right-hand sides along.  Both recursions run
// from the last knot to the first, the sweep's stage i needs nothing but what the factor's stage i holds in registers at its end --
// K_i[:, c], H_i^-1, dt_i, column c of [A B]_i (lane (r, c) of the factor IS lane (s, c) of the sweep: s = DPP row parity) -- and the
// right-hand side, and its ~30 instructions sit in the shadows of the factor's LDS exchanges: an iteration is four dependent chains
// over the horizon instead of five.  The right-hand side must then exist BEFORE the factorisation: the iteration assembles the
// predictor's gradient first (it depends on the iterate only) into the rhs0 cells, and the barrier weights the factor reads move
// to the rhs1 cells (`th_off` = KN_R1, the boundary row's weight to `tey_off` = KN_TEY) -- the Schur vector that used to sit there
// is one number per knot (c_sigma on e_y: KN_CSIG), generated on the fly.  The arithmetic of either recursion is the unfused one's,
// operation for operation.  riccati_solve<.., 2, true> then runs the forward half only.
#define KN_TEY 35  // (the knot record's spare cell)
// CHAIN_PINNED (lmpc_chain_addr, lmpc_solve_layout.hip.h): what the loop reads and writes in the stage and knot records -- the cells that
// move from stage to stage; P, W, Y in the tail stay where they are -- goes through LDS byte addresses, one per lane pattern, each
// advanced once per stage, every access at a compile-time offset from one of them: the same cells in the same order.
template <ChainForm FORM, bool HAS_PT, bool JOSEPH, bool FUSE = false, typename real, typename ptreal>
__device__ __forceinline__ void riccati_factor(const Lds<real>& L, ModelStream<real>& MS, int lane, const ptreal* PT, const int th_off = KN_R0, const int tey_off = KN_EY) {
  typedef StageCells<FORM> SC;
  FRESH_LANE(lane);
  if constexpr (SC::prio) CHAIN_PRIO_ENTER();
  const int N = L.N, r = lane >> 3, c = lane & 7;
  real* T = L.tail();
  real* MP = T + TL_P;
  real* MW = T + TL_W;
  real* MY = T + TL_Y;
  const real* ct = T + TL_CT;
  const bool diag = r == c;
  // per-lane 0/1 multipliers instead of selects (exact: the products are the operand or zero)
  const real m_diag = diag ? real(1) : real(0), m_r1 = r == 1 ? real(1) : real(0);
  const real m_r6 = r >= 6 ? real(1) : real(0), m_c6 = c >= 6 ? real(1) : real(0);
  const real qmid = qz_entry(ct, false, r, c);
  real pown;
  {
    int ch = 0;
    if constexpr (SC::lean) {  // (the chunk the sweep starts in is requested ...)
      ch = (N - 2) / LN_CHUNK;
      MS.ensure(ch);
    }
    const real* kn = L.kn(N - 1);
    real e = qz_entry(ct, true, r, c);
    const real th = kn[th_off + r] + (r == 1 ? kn[tey_off] : real(0));
    if (diag) e += th;
    // LMPC: safe-set block condensed onto x_T; its upper triangle is the block (see the symmetry note in the loop)
    if (HAS_PT && r < 6 && c < 6) e += real(PT[r <= c ? r * 6 + c : c * 6 + r]);
    pown = e;
    MP[MROWS(r) + c] = e;
    if constexpr (SC::lean) {  // (... and there; the one below it is requested at once)
      MS.wait();
      if (ch > 0) MS.ensure(ch - 1);
    }
  }
  // fused backward sweep: lane (s, c), s = parity of the DPP row; rhs0 = the knots' rhs0 cells, rhs1 = c_sigma e_y (knots >= 1)
  const int fs = (lane >> 4) & 1;
  const bool f_own = FUSE && (lane & 8) == 0 && lane < 32 && c < 2;
  const int f_oq = fs == 0 ? KN_R0 + c : KN_CSIG;                       // where the sweep's q_z comes from ...
  const real f_mq = (fs == 0 || c == 1) ? real(1) : real(0);            // ... and whether it counts
  const real f_m6 = (c >= 6) ? real(1) : real(0);
  real fp = 0.0, fws = 0.0, fw6 = 0.0, fw7 = 0.0, fqz = 0.0, fqv0 = 0.0, fqv1 = 0.0;
  if constexpr (FUSE) fp = f_mq * L.kn(N - 1)[f_oq];
  // The upper triangle (lanes r <= c) is the cost-to-go; those lanes store their element at (r, c) AND (c, r), the others
  // store to a dead cell.  Why: the two computed halves differ by rounding, and that antisymmetric part is not contracted by
  // the recursion -- it is multiplied by Abar'(.)Abar, the OPEN-loop dynamics, whose RK4 map has |eig| up to ~15-25 below
  // 1 m/s, so within twenty stages it reaches 1e17 and the Newton directions are noise (every low-speed cold start at
  // N >= 40 was lost to this).  An exactly symmetric P only carries symmetric error, which the closed loop damps.
  const bool upper = r <= c;
  real* const p_dst0 = upper ? MP + MROWS(r) + c : MW + MROWS(r) + c;
  real* const p_dst1 = upper ? MP + MROWS(c) + r : MW + MROWS(r) + c;
  // where this lane's share of the stage results goes: lanes 0..15 K_j[c] (j = r), 16..18 Hinv, the
  // rest to their own (dead) W cell
  const int res_off = lane < 16 ? SC::krow(c) + SC::kidx + r : (lane == 18 ? SC::hi11 : SC::hi + (lane - 16));
  const bool res_on = lane < 19;
  real* const res_junk = MW + MROWS(r) + c;
  // phase-1/2 operands of stage N-2 (later stages: fetched during phase 3 of the stage before)
  real ar[6], ac[6];
  {
    const real* ab = SC::model(L, MS, N - 2);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      ar[k] = ab[SC::row(r) + k];
      ac[k] = ab[SC::row(c) + k];
    }
  }
  // the input-rate weights are the same at every stage: scalar registers, not an LDS read per stage
  const real sv00 = uni(ct[CT_SV + 0]), sv01 = uni(ct[CT_SV + 1]), sv11 = uni(ct[CT_SV + 3]);
  wave_sync();
  real pr[6];
  if constexpr (FUSE) {  // (fused: the P row of a stage is requested at the end of the stage before, ahead of the sweep's share of it)
#pragma unroll
    for (int k = 0; k < 6; ++k) pr[k] = MP[MROWS(c) + k];
    pown = MP[MROWS(r) + c];
    ISSUE_ORDER();
  }
  // CHAIN_PINNED: wave-uniform cells of the stage and of the knot, the knot's weight by row, the sweep's q_z, the rows r and c of the
  // stage fetched ahead (stride 0 once it is stage 0), and the two store targets (a dead cell: stride 0)
  unsigned a_stu = 0, a_knu = 0, a_thr = 0, a_foq = 0, a_nr = 0, a_nc = 0, a_res = 0, a_kff = 0, s_res = 0, s_kff = 0;
  constexpr unsigned ca_kb = LMPC_KNOT_STRIDE * sizeof(real);
  const unsigned ca_sb = L.stride * sizeof(real);
  if constexpr (SC::pinned) {
    const int in = N > 2 ? N - 3 : 0;
    a_stu = lds_addr(L.st(N - 2));
    a_knu = lds_addr(L.kn(N - 2));
    a_thr = lds_addr(L.kn(N - 2) + th_off + r);
    a_foq = lds_addr(L.kn(N - 2) + f_oq);
    a_nr = lds_addr(L.st(in) + ST_ROW(r));
    a_nc = lds_addr(L.st(in) + ST_ROW(c));
    a_res = lds_addr(res_on ? L.st(N - 2) + res_off : res_junk);
    a_kff = lds_addr(f_own ? L.st(N - 2) + ST_KFF(fs) + c : res_junk);
    s_res = res_on ? ca_sb : 0u;
    s_kff = f_own ? ca_sb : 0u;
  }
  for (int i = N - 2; i >= 0; --i) {
    real* st = L.st(i);
    const real* kn = L.kn(i);
    const real* ab = SC::model(L, MS, i);
    const bool cross = SC::lean && (i % LN_CHUNK) == 0 && i > 0;  // the read-ahead of this stage is the first read of the chunk below
    if constexpr (SC::pinned) {
      CHAIN_ADDR_PIN16(a_stu); CHAIN_ADDR_PIN16(a_knu); CHAIN_ADDR_PIN(a_thr); CHAIN_ADDR_PIN16(a_nr); CHAIN_ADDR_PIN16(a_nc); CHAIN_ADDR_PIN(a_res);
      if constexpr (FUSE) { CHAIN_ADDR_PIN(a_foq); CHAIN_ADDR_PIN(a_kff); }
    }
    // W = Abar' P : W[r][c] = sum_k Abar[k][r] P[k][c]  (+ P[r][c] for the u rows); P[k][c] read as P[c][k]
    if constexpr (!FUSE) {
#pragma unroll
      for (int k = 0; k < 6; ++k) pr[k] = MP[MROWS(c) + k];
      pown = MP[MROWS(r) + c];  // the symmetrised element (lanes below the diagonal did not compute it)
      ISSUE_ORDER();
    }
    // phase-3 operands of this stage, queued behind the P row
    const real t = CHAIN_GET(a_stu, st, 0, SC::dt), thr = CHAIN_GET(a_thr, kn, th_off + r, 0), ey = CHAIN_GET(a_knu, kn, 0, tey_off), thv0 = CHAIN_GET(a_knu, kn, 0, th_off + 8), thv1 = CHAIN_GET(a_knu, kn, 0, th_off + 9);
    if constexpr (FUSE) {
      fqz = CHAIN_GET(a_foq, kn, f_oq, 0);
      fqv0 = CHAIN_GET(a_knu, kn, 0, KN_R0 + 8);
      fqv1 = CHAIN_GET(a_knu, kn, 0, KN_R0 + 9);
    }
    ISSUE_ORDER();
    real w = m_r6 * pown;
#pragma unroll
    for (int k = 0; k < 6; ++k) w += ar[k] * pr[k];
    MW[MROWS(r) + c] = w;
    wave_sync();
    // Y = W Abar
    real wr[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) wr[k] = MW[MROWS(r) + k];
    if constexpr (FUSE) {  // the sweep's w = Abar' p (+ p_u on the input rows), while the W row is on its way; ac = [A B](:, c)
      ISSUE_ORDER();
      real pb[6];
      row_bcast6(fp, pb);
      fws = f_m6 * fp;
#pragma unroll
      for (int k = 0; k < 6; ++k) fws = rfma(ac[k], pb[k], fws);
      row_bcast67(fws, fw6, fw7);
    }
    real y = m_c6 * w;
#pragma unroll
    for (int k = 0; k < 6; ++k) y += wr[k] * ac[k];
    MY[MROWS(r) + c] = y;
    wave_sync();
    // H = Sv + Thv + t^2 Y_uu, K = H^-1 t Y[6:8,:], P <- Qz + Thz + Y - t^2 Y[6:8,r]' H^-1 Y[6:8,c]
    const real y6r = MY[MROWS(6) + r], y7r = MY[MROWS(7) + r];
    const real y6c = MY[MROWS(6) + c], y7c = MY[MROWS(7) + c];
    AFTER_VALUE(y);
    // phase-1/2 operands of the next stage (their registers are dead by now), queued behind the Y rows
    if constexpr (!JOSEPH) {
      if constexpr (SC::lean) if (cross) MS.wait();
      const real* abn = SC::pinned ? nullptr : SC::model(L, MS, i > 0 ? i - 1 : 0);  // (pinned: the addresses are there already)
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        ar[k] = CHAIN_GET(a_nr, abn, SC::row(r), k);
        ac[k] = CHAIN_GET(a_nc, abn, SC::row(c), k);
      }
      if constexpr (SC::lean) if (cross && i / LN_CHUNK >= 2) {  // (the chunk just left is dead: the one after into its buffer)
        wave_fence();
        MS.fetch(i / LN_CHUNK - 2);
      }
    }
    ISSUE_ORDER();
    const real y66 = lane_bcast(y, 54), y67 = lane_bcast(y, 55), y77 = lane_bcast(y, 63);
    const real tt = t * t;
    const real h00 = sv00 + thv0 + tt * y66;
    const real h01 = sv01 + tt * y67;
    const real h11 = sv11 + thv1 + tt * y77;
    real idet;
    if constexpr (sizeof(real) == 4) {
      // H = R + t^2 Y_uu is rank-one dominated once a state row is stiff: its determinant is the difference of two
      // products that agree to six digits, which single precision cannot form -- a handful of fp64 operations per stage
      const double det = (double)h00 * (double)h11 - (double)h01 * (double)h01;
      idet = (real)(1.0 / det);
    } else {
      idet = frcp(h00 * h11 - h01 * h01);
    }
    const real hi00 = h11 * idet, hi01 = -h01 * idet, hi11 = h00 * idet;
    const real g0 = t * y6c, g1 = t * y7c;
    const real k0c = hi00 * g0 + hi01 * g1;
    const real k1c = hi01 * g0 + hi11 * g1;
    real pn;
    if constexpr (JOSEPH) {
      // the gain at this lane's ROW index as well: K[:, r] from Y[6:8, r], the same expression lane (., r) evaluates
      const real g0r = t * y6r, g1r = t * y7r;
      const real k0r = hi00 * g0r + hi01 * g1r;
      const real k1r = hi01 * g0r + hi11 * g1r;
      // columns r and c of Phi (overwriting the columns of Abar they are made from); B = Abar[:, 6:8] as broadcast reads
      {
        real b0[6], b1[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          b0[k] = CHAIN_GET(a_stu, ab, 0, SC::row(6) + k);
          b1[k] = CHAIN_GET(a_stu, ab, 0, SC::row(7) + k);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          ar[k] -= t * (b0[k] * k0r + b1[k] * k1r);
          ac[k] -= t * (b0[k] * k0c + b1[k] * k1c);
        }
      }
      const real fr6 = (r == 6 ? real(1) : real(0)) - t * k0r, fr7 = (r == 7 ? real(1) : real(0)) - t * k1r;
      const real fc6 = (c == 6 ? real(1) : real(0)) - t * k0c, fc7 = (c == 7 ? real(1) : real(0)) - t * k1c;
      // W2 = Phi' P (P symmetric: P[k][c] read as P[c][k]), exchanged through the W matrix (its phase-2 reads are done)
      real w2 = 0.0;
      {
        real pc[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) pc[k] = MP[MROWS(c) + k];
#pragma unroll
        for (int k = 0; k < 6; ++k) w2 += ar[k] * pc[k];
        w2 += fr6 * pc[6] + fr7 * pc[7];
      }
      MW[MROWS(r) + c] = w2;
      wave_sync();
      real y2 = 0.0;
      {
        real w2r[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) w2r[k] = MW[MROWS(r) + k];
#pragma unroll
        for (int k = 0; k < 6; ++k) y2 += w2r[k] * ac[k];
        y2 += w2r[6] * fc6 + w2r[7] * fc7;
      }
      {
        if constexpr (SC::lean) if (cross) MS.wait();
        const real* abn = SC::pinned ? nullptr : SC::model(L, MS, i > 0 ? i - 1 : 0);  // (pinned: the addresses are there already)
  #pragma unroll
        for (int k = 0; k < 6; ++k) {
          ar[k] = CHAIN_GET(a_nr, abn, SC::row(r), k);
          ac[k] = CHAIN_GET(a_nc, abn, SC::row(c), k);
        }
        if constexpr (SC::lean) if (cross && i / LN_CHUNK >= 2) {  // (the chunk just left is dead: the one after into its buffer)
        wave_fence();
        MS.fetch(i / LN_CHUNK - 2);
      }
      }
      const real v00 = sv00 + thv0, v11 = sv11 + thv1;
      pn = qmid + y2 + k0r * (v00 * k0c + sv01 * k1c) + k1r * (sv01 * k0c + v11 * k1c);
    } else {
      pn = qmid + y - t * (y6r * k0c + y7r * k1c);
    }
    const real th = rfma(m_r1, ey, thr);
    pn = rfma(m_diag, th, pn);
    *p_dst0 = pn;  // (not used after stage 0)
    *p_dst1 = pn;
    const real res = lane < 8 ? k0c : (lane < 16 ? k1c : (lane == 16 ? hi00 : (lane == 17 ? hi01 : hi11)));
    CHAIN_PUT(a_res, res_on ? st + res_off : res_junk, res);
    wave_sync();
    if constexpr (FUSE) {
      if (i > 0) {  // the next stage's P row, behind the stores above
#pragma unroll
        for (int k = 0; k < 6; ++k) pr[k] = MP[MROWS(c) + k];
        pown = MP[MROWS(r) + c];
      }
      ISSUE_ORDER();
      // the sweep's stage i: p_i = q_i + Abar' p_{i+1} - K' (q_v + Bbar' p_{i+1}),  kff_i = H^-1 (q_v + Bbar' p_{i+1})
      const real qv0 = fs == 0 ? fqv0 : real(0), qv1 = fs == 0 ? fqv1 : real(0);
      const real hv0 = rfma(t, fw6, qv0);
      const real hv1 = rfma(t, fw7, qv1);
      fp = f_mq * fqz + fws - (k0c * hv0 + k1c * hv1);
      const real ha = c == 0 ? hi00 : hi01, hb = c == 0 ? hi01 : hi11;
      const real kff = ha * hv0 + hb * hv1;
      CHAIN_PUT(a_kff, f_own ? st + SC::kff(fs) + c : res_junk, kff);
    }
    if constexpr (SC::pinned) {
      const unsigned s_nxt = i >= 2 ? ca_sb : 0u;  // (the fetch ahead stops at stage 0)
      a_stu -= ca_sb; a_knu -= ca_kb; a_thr -= ca_kb; a_res -= s_res; a_nr -= s_nxt; a_nc -= s_nxt;
      if constexpr (FUSE) { a_foq -= ca_kb; a_kff -= s_kff; }
    }
  }
  if constexpr (FUSE)
    wave_sync();  // (what follows is the forward half of the solve: lean, chunks 0 and 1 are what the factor ended on)
  else if constexpr (SC::lean) {
    if ((N - 2) / LN_CHUNK >= 2) {
      // what follows is a vector solve, whose backward sweep starts at the top again: its first chunks are on their way while
      // the gradient is assembled (both buffers are free: the factor is done with them)
      MS.fetch((N - 2) / LN_CHUNK);
      MS.fetch((N - 2) / LN_CHUNK - 1);
    }
  }
  if constexpr (SC::prio) CHAIN_PRIO_LEAVE();
}

// Riccati vector solve for NRHS (1 or 2) right-hand sides held in the knots' rhs regions
// (q_z @ +0..7, q_v @ +8,9 of region s); the step (dz, dv) overwrites them.  dz_0 = 0.
//
// Both sweeps are strictly serial over the knots: one dependent chain of N - 1 stages each, and the chain's length, not
// the instruction count, is what a solve waits for.  Lane (s, r) = ((lane >> 4) % NRHS, lane & 7): each right-hand side
// has a 16-lane DPP row of its own (lanes 8..15 of a row, and the rows above NRHS, mirror lanes below and write to dead
// cells), the running vector lives in ONE register per lane, and a stage gets the other components by row_newbcast --
// nothing on the chain goes through LDS (it did until round 2: one write + broadcast reads per stage, and a ds_swizzle
// for the condensed 2-vector; ~400 cycles per stage under load).  Stage operands are fetched one stage ahead; the
// results a stage leaves behind (kff, dz, dv) are stored off the chain.
// CHAIN_ADDR (lmpc_chain_addr, lmpc_solve_layout.hip.h): the stage loops walk LDS byte addresses, one per lane pattern, each advanced
// once per stage, and every access of a stage is a compile-time offset from one of them -- the same cells in the same order.
template <int NRHS, bool FWD_ONLY = false, bool CHAIN_ADDR = false, typename real>  // (FWD_ONLY: the backward half ran inside the factorisation, riccati_factor<.., FUSE>)
__device__ __forceinline__ void riccati_solve_fat(const Lds<real>& L, int lane, Prof& pf) {
  FRESH_LANE(lane);
  CHAIN_PRIO_ENTER();
  const int N = L.N;
  const int r = lane & 7, s = (lane >> 4) & (NRHS - 1);
  const bool own = (lane & 8) == 0 && lane < 16 * NRHS;
  const int reg = KN_R0 + 10 * s;
  real* T = L.tail();
  real* const junk0 = T + TL_W + lane;  // 64 + 64 dead cells: W (80) and Y (80) are contiguous
  real* const junk1 = T + TL_W + 80 + lane;
  const real m6 = (r >= 6) ? real(1) : real(0);  // rows 6, 7 (the input rows of z) take an extra term: a multiplier, not a select
  // kff = H^-1 hv: lane r = 0 takes row (h00, h01), the others row (h01, h11) -- picked by the address, not by a select
  const int o_ha = r == 0 ? ST_HI : ST_HI + 1, o_hb = r == 0 ? ST_HI + 1 : ST_HI11;
  // ---- backward: p_i = q_i + Abar' p_{i+1} - K' (q_v + Bbar' p_{i+1});  kff_i = H^-1 (q_v + Bbar' p_{i+1})
  real p = FWD_ONLY ? real(0) : L.kn(N - 1)[reg + r];
  real row[6];  // [A B](:, r), fetched one stage ahead
  if constexpr (!FWD_ONLY) {
    const real* st = L.st(N - 2);
#pragma unroll
    for (int k = 0; k < 6; ++k) row[k] = st[ST_ROW(r) + k];
  }
  if constexpr (CHAIN_ADDR && !FWD_ONLY) {
    const unsigned sb = L.stride * sizeof(real), kb = LMPC_KNOT_STRIDE * sizeof(real);
    const bool kown = own && r < 2;
    unsigned a_row = lds_addr(L.st(N - 2) + ST_ROW(r));                 // row-indexed: K(:, r) of this stage
    unsigned a_nxt = lds_addr(L.st(N > 2 ? N - 3 : 0) + ST_ROW(r));     // ... and [A B](:, r) of the stage fetched ahead
    unsigned a_uni = lds_addr(L.st(N - 2));                             // wave-uniform: dt
    unsigned a_ha = lds_addr(L.st(N - 2) + o_ha), a_hb = lds_addr(L.st(N - 2) + o_hb);
    unsigned a_qz = lds_addr(L.kn(N - 2) + reg + r);                    // knot-indexed: q_z by lane, q_v by right-hand side
    unsigned a_qv = lds_addr(L.kn(N - 2) + reg);
    unsigned a_kff = lds_addr(kown ? L.st(N - 2) + ST_KFF(s) + r : junk1);  // store target (a dead cell: stride 0)
    const unsigned s_kff = kown ? sb : 0u;
    for (int i = N - 2; i >= 0; --i) {
      CHAIN_ADDR_PIN16(a_row); CHAIN_ADDR_PIN16(a_nxt); CHAIN_ADDR_PIN(a_uni); CHAIN_ADDR_PIN(a_ha);
      CHAIN_ADDR_PIN(a_hb); CHAIN_ADDR_PIN(a_qz); CHAIN_ADDR_PIN16(a_qv); CHAIN_ADDR_PIN(a_kff);
      const LMPC_LDS real* const p_row = lds_at<real>(a_row);
      const LMPC_LDS real* const p_nxt = lds_at<real>(a_nxt);
      const LMPC_LDS real* const p_qv = lds_at<real>(a_qv);
      const real k0r = p_row[6], k1r = p_row[7], t = lds_at<real>(a_uni)[ST_DT];
      const real qz = *lds_at<real>(a_qz), qv0 = p_qv[8], qv1 = p_qv[9];
      const real ha = *lds_at<real>(a_ha), hb = *lds_at<real>(a_hb);
      real pb[6];
      row_bcast6(p, pb);
      real w = m6 * p;
#pragma unroll
      for (int k = 0; k < 6; ++k) w = rfma(row[k], pb[k], w);
      real w6, w7;
      row_bcast67(w, w6, w7);
#pragma unroll
      for (int k = 0; k < 6; ++k) row[k] = p_nxt[k];
      const real hv0 = rfma(t, w6, qv0);
      const real hv1 = rfma(t, w7, qv1);
      p = qz + w - (k0r * hv0 + k1r * hv1);
      const real kff = ha * hv0 + hb * hv1;
      *lds_at<real>(a_kff) = kff;
      a_row -= sb; a_uni -= sb; a_ha -= sb; a_hb -= sb; a_qz -= kb; a_qv -= kb; a_kff -= s_kff;
      a_nxt -= i >= 2 ? sb : 0u;  // (the fetch ahead stops at stage 0)
    }
  } else
  for (int i = FWD_ONLY ? -1 : N - 2; i >= 0; --i) {
    real* st = L.st(i);
    const real* kn = L.kn(i);
    const real k0r = st[ST_ROW(r) + 6], k1r = st[ST_ROW(r) + 7], t = st[ST_DT];
    const real qz = kn[reg + r], qv0 = kn[reg + 8], qv1 = kn[reg + 9];
    const real ha = st[o_ha], hb = st[o_hb];
    real pb[6];
    row_bcast6(p, pb);
    real w = m6 * p;  // w = Abar' p: rows 6,7 also take p_u
#pragma unroll
    for (int k = 0; k < 6; ++k) w = rfma(row[k], pb[k], w);
    real w6, w7;
    row_bcast67(w, w6, w7);
    {
      const real* stn = L.st(i > 0 ? i - 1 : 0);
#pragma unroll
      for (int k = 0; k < 6; ++k) row[k] = stn[ST_ROW(r) + k];
    }
    const real hv0 = rfma(t, w6, qv0);
    const real hv1 = rfma(t, w7, qv1);
    p = qz + w - (k0r * hv0 + k1r * hv1);  // (not used after stage 0)
    const real kff = ha * hv0 + hb * hv1;
    *((own && r < 2) ? st + ST_KFF(s) + r : junk1) = kff;
  }
  wave_sync();
  PT_MARK(8 + NRHS - 1)
  // ---- forward: dv_i = -kff_i - K dz_i,  dz_{i+1} = Abar dz_i + Bbar dv_i
  // lanes r < 6 take a state row, lanes 6, 7 the two rows of K: column k of M is [A B](:, k) | K(:, k)
  *(own ? L.kn(0) + reg + r : junk0) = 0.0;
  real d = 0.0;     // component r of dz_i
  real col[8], a0;  // M(r, :) and the feed-forward term, fetched one stage ahead
  {
    const real* st = L.st(0);
#pragma unroll
    for (int k = 0; k < 8; ++k) col[k] = st[ST_ROW(k) + r];
    a0 = st[ST_KFF(s) + (r & 1)];
  }
  if constexpr (CHAIN_ADDR) {
    const unsigned sb = L.stride * sizeof(real);
    unsigned a_col = lds_addr(L.st(0) + r);                      // column-indexed: Bbar(r, :) of this stage
    unsigned a_nxt = lds_addr(L.st(N > 2 ? 1 : 0) + r);          // ... and M(r, :) of the stage fetched ahead
    unsigned a_kff = lds_addr(L.st(N > 2 ? 1 : 0) + ST_KFF(s) + (r & 1));
    unsigned a_uni = lds_addr(L.st(0));                          // wave-uniform: dt
    unsigned a_dz = lds_addr(own ? L.kn(1) + reg + r : junk0);   // store targets (a dead cell: stride 0)
    unsigned a_dv = lds_addr((own && r >= 6) ? L.kn(0) + reg + 2 + r : junk1);
    const unsigned s_dz = own ? unsigned(LMPC_KNOT_STRIDE * sizeof(real)) : 0u;
    const unsigned s_dv = (own && r >= 6) ? unsigned(LMPC_KNOT_STRIDE * sizeof(real)) : 0u;
    for (int i = 0; i < N - 1; ++i) {
      CHAIN_ADDR_PIN(a_col); CHAIN_ADDR_PIN(a_nxt); CHAIN_ADDR_PIN(a_kff);
      CHAIN_ADDR_PIN(a_uni); CHAIN_ADDR_PIN(a_dz); CHAIN_ADDR_PIN(a_dv);
      const LMPC_LDS real* const p_col = lds_at<real>(a_col);
      const LMPC_LDS real* const p_nxt = lds_at<real>(a_nxt);
      const real b0 = p_col[ST_ROW(6)], b1 = p_col[ST_ROW(7)], t = lds_at<real>(a_uni)[ST_DT];
      real dz[8];
      row_bcast8(d, dz);
      real acc = m6 * a0;
#pragma unroll
      for (int k = 0; k < 6; ++k) acc = rfma(col[k], dz[k], acc);
      const real ax = acc;
      acc = rfma(col[6], dz[6], acc);
      acc = rfma(col[7], dz[7], acc);
      const real dv = -acc;
      const real du = rfma(t, dv, d);
      real du0, du1;
      row_bcast67(du, du0, du1);
#pragma unroll
      for (int k = 0; k < 8; ++k) col[k] = p_nxt[ST_ROW(k)];
      a0 = *lds_at<real>(a_kff);
      const real nx = rfma(b1, du1, rfma(b0, du0, ax));
      d = (r < 6) ? nx : du;
      *lds_at<real>(a_dz) = d;
      *lds_at<real>(a_dv) = dv;
      a_col += sb; a_uni += sb; a_dz += s_dz; a_dv += s_dv;
      const unsigned s_nxt = i < N - 3 ? sb : 0u;  // (the fetch ahead stops at the last stage)
      a_nxt += s_nxt; a_kff += s_nxt;
    }
  } else
  for (int i = 0; i < N - 1; ++i) {
    const real* st = L.st(i);
    real* kn = L.kn(i);
    const real b0 = st[ST_ROW(6) + r], b1 = st[ST_ROW(7) + r], t = st[ST_DT];
    real dz[8];
    row_bcast8(d, dz);
    real acc = m6 * a0;
#pragma unroll
    for (int k = 0; k < 6; ++k) acc = rfma(col[k], dz[k], acc);
    const real ax = acc;  // state rows: A dz_x
    acc = rfma(col[6], dz[6], acc);
    acc = rfma(col[7], dz[7], acc);
    const real dv = -acc;  // lanes 6, 7
    const real du = rfma(t, dv, d);  // (lanes 6, 7: their own component of dz is u_{i-1})
    real du0, du1;
    row_bcast67(du, du0, du1);
    {
      const real* stn = L.st(i < N - 2 ? i + 1 : i);
#pragma unroll
      for (int k = 0; k < 8; ++k) col[k] = stn[ST_ROW(k) + r];
      a0 = stn[ST_KFF(s) + (r & 1)];
    }
    const real nx = rfma(b1, du1, rfma(b0, du0, ax));
    d = (r < 6) ? nx : du;
    *(own ? kn + LMPC_KNOT_STRIDE + reg + r : junk0) = d;
    *((own && r >= 6) ? kn + reg + 2 + r : junk1) = dv;
  }
  wave_sync();
  CHAIN_PRIO_LEAVE();
  PT_MARK(10 + NRHS - 1)
}

// The lean vector solve with the running vector in registers (DPP row broadcasts, as riccati_solve_fat) instead of one LDS round
// trip per stage: at one wave per SIMD a sweep stage costs what its instruction count costs (~4.5 cycles each, nothing to
// overlap with), and the exchange through LDS was a third of the lean stage's instructions (the LDS-exchange form of rounds 2-3,
// bit for bit the same results, is scratch/r5/experiment_switches.patch); lane (s, r) = ((lane >> 4) % NRHS, lane & 7), lanes 8..15 of a row mirror 0..7.
template <int NRHS, bool FWD_ONLY = false, typename real>
__device__ __forceinline__ void riccati_solve_lean(const Lds<real>& L, ModelStream<real>& M, int lane, Prof& pf) {
  FRESH_LANE(lane);
  const int N = L.N;
  const int r = lane & 7, s = (lane >> 4) & (NRHS - 1);
  const bool own = (lane & 8) == 0 && lane < 16 * NRHS;
  const int reg = KN_R0 + 10 * s;
  real* T = L.tail();
  real* const junk0 = T + TL_W + lane;
  real* const junk1 = T + TL_W + 80 + lane;
  const real m6 = (r >= 6) ? real(1) : real(0);
  const int o_ha = r == 0 ? LN_HI : LN_HI + 1, o_hb = r == 0 ? LN_HI + 1 : LN_HI11;
  // ---- backward
  if constexpr (!FWD_ONLY) {
    const int ch = (N - 2) / LN_CHUNK;
    M.ensure(ch);
    M.wait();
    if (ch > 0) M.ensure(ch - 1);
  }
  real p = FWD_ONLY ? real(0) : L.kn(N - 1)[reg + r];
  real row[6];
  if constexpr (!FWD_ONLY) {
    const real* ab = M.stage(N - 2);
#pragma unroll
    for (int k = 0; k < 6; ++k) row[k] = ab[6 * r + k];
  }
  for (int i = FWD_ONLY ? -1 : N - 2; i >= 0; --i) {
    real* st = L.st(i);
    const real* kn = L.kn(i);
    if ((i % LN_CHUNK) == 0 && i > 0) {  // (chunk boundary: the next chunk must have landed)
      M.wait();
      if (i / LN_CHUNK >= 2) M.fetch(i / LN_CHUNK - 2);
    }
    const real k0r = st[2 * r], k1r = st[2 * r + 1], t = st[LN_DT];
    const real qz = kn[reg + r], qv0 = kn[reg + 8], qv1 = kn[reg + 9];
    const real ha = st[o_ha], hb = st[o_hb];
    real pb[6];
    row_bcast6(p, pb);
    real w = m6 * p;
#pragma unroll
    for (int k = 0; k < 6; ++k) w = rfma(row[k], pb[k], w);
    real w6, w7;
    row_bcast67(w, w6, w7);
    {
      const real* abn = M.stage(i > 0 ? i - 1 : 0);
#pragma unroll
      for (int k = 0; k < 6; ++k) row[k] = abn[6 * r + k];
    }
    const real hv0 = rfma(t, w6, qv0);
    const real hv1 = rfma(t, w7, qv1);
    p = qz + w - (k0r * hv0 + k1r * hv1);
    const real kff = ha * hv0 + hb * hv1;
    *((own && r < 2) ? st + LN_KFF(s) + r : junk1) = kff;
  }
  wave_sync();
  PT_MARK(8 + NRHS - 1)
  // ---- forward
  const int nch = (N - 2) / LN_CHUNK + 1;
  M.ensure(0);
  *(own ? L.kn(0) + reg + r : junk0) = 0.0;
  M.wait();
  if (nch > 1) M.ensure(1);
  const int cb = r < 6 ? r : 0;
  const int cstride = r < 6 ? 6 : 2;
  real d = 0.0;
  real col[8], a0, b0n, b1n;
  auto load_stage = [&](int i) {
    const real* ab = M.stage(i);
    const real* st = L.st(i);
    {
      const real* const cbase = r < 6 ? ab + cb : st + (r - 6);
#pragma unroll
      for (int k = 0; k < 8; ++k) col[k] = cbase[k * cstride];
    }
    a0 = st[LN_KFF(s) + (r & 1)];
    b0n = ab[36 + cb];
    b1n = ab[42 + cb];
  };
  load_stage(0);
  wave_sync();
  for (int i = 0; i < N - 1; ++i) {
    const real* st = L.st(i);
    real* kn = L.kn(i);
    if ((i % LN_CHUNK) == LN_CHUNK - 1 && i < N - 2) {
      M.wait();
      if (i / LN_CHUNK + 2 < nch) M.fetch(i / LN_CHUNK + 2);
    }
    const real b0 = b0n, b1 = b1n, t = st[LN_DT];
    real dz[8];
    row_bcast8(d, dz);
    real acc = m6 * a0;
#pragma unroll
    for (int k = 0; k < 6; ++k) acc = rfma(col[k], dz[k], acc);
    const real ax = acc;
    acc = rfma(col[6], dz[6], acc);
    acc = rfma(col[7], dz[7], acc);
    const real dv = -acc;
    const real du = rfma(t, dv, d);
    real du0, du1;
    row_bcast67(du, du0, du1);
    load_stage(i < N - 2 ? i + 1 : i);
    const real nx = rfma(b1, du1, rfma(b0, du0, ax));
    d = (r < 6) ? nx : du;
    *(own ? kn + LMPC_KNOT_STRIDE + reg + r : junk0) = d;
    *((own && r >= 6) ? kn + reg + 2 + r : junk1) = dv;
  }
  wave_sync();
  PT_MARK(10 + NRHS - 1)
}

// The vector solve in the form of the instantiation.  NOT one body yet, unlike the factorisation and the rollout: merged with the
// accessors of lmpc_solve_layout.hip.h the indexed form compiles to the separate function's code, but the pinned and the lean form do
// not (the lean forward sweep's fetch of a stage is a lambda that captures its arrays, the fat one's is written out, and the optimiser
// treats the two differently), so the two functions above stay as they were and this only picks one.
template <ChainForm FORM, int NRHS, bool FWD_ONLY = false, typename real>
__device__ __forceinline__ void riccati_solve(const Lds<real>& L, ModelStream<real>& MS, int lane, Prof& pf) {
  if constexpr (FORM == CHAIN_LEAN)
    riccati_solve_lean<NRHS, FWD_ONLY>(L, MS, lane, pf);
  else
    riccati_solve_fat<NRHS, FWD_ONLY, FORM == CHAIN_PINNED>(L, lane, pf);
}

// Closed-loop rollout z_{i+1} = Abar z_i + Bbar v_i + gbar, v_i = -K_i z_i (absolute variables).
// The linearised model can be open-loop unstable (|eig A| > 1 at low speed with dt = 25 ms), so
// the start trajectory is generated under the stabilising Riccati feedback.  Same lane roles as the
// forward sweep of riccati_solve.
// WARM (lmpc_solve_batch_warm): the rollout TRACKS a plan -- v_i = v_i^plan - K_i (z_i - z_i^plan) -- whose knots sit in the rhs0
// cells of the knot records ([z^plan (8) | v^plan (2)] at KN_R0: free between the factorisation that has read its weights
// there and the first gradient): the plan made dynamically exact about this linearisation, a few 1e-3 from where it was.
// Two algorithms.  CHAIN_INDEXED and CHAIN_LEAN share the LDS-exchange loop at the bottom: z_i is read back from the knot record
// every stage, one wave_sync() per stage.  CHAIN_PINNED is a body of its own, the forward sweep's form: component r of z_i stays in
// one register per lane and reaches the other lanes by row_newbcast; M(r, :), g, dt -- and the plan's knot of a WARM rollout -- of
// stage i + 1 are fetched during stage i through addresses that advance once per stage (stride 0 once the fetch ahead has reached
// the last stage); z_{i+1} and v_i are stored off the chain (a dead cell: stride 0), so nothing a stage reads was written by the
// loop and the one wave_sync() is at the end.  The arithmetic is the loop's below, operation for operation.
template <ChainForm FORM, bool WARM = false, typename real>
__device__ __forceinline__ void feedback_rollout(const Lds<real>& L, ModelStream<real>& MS, int lane) {
  typedef StageCells<FORM> SC;
  FRESH_LANE(lane);
  const int N = L.N, r = lane & 7;
  const bool own = lane < 8;
  real* T = L.tail();
  real* const junk0 = T + TL_W + lane;
  real* const junk1 = T + TL_W + 80 + lane;
  if constexpr (SC::pinned) {
    const unsigned sb = L.stride * sizeof(real);
    constexpr unsigned kb = LMPC_KNOT_STRIDE * sizeof(real);
    const int o_g = ST_G + (r < 6 ? r : 0);
    real d = L.kn(0)[r];  // component r of z_i
    real col[8], t, g;    // M(r, :), dt and g of the stage: fetched one stage ahead
    real pl[8], pv = 0.0; // WARM: the plan's knot, z^plan (wave-uniform) and this lane's v^plan
    {
      const real* st = L.st(0);
#pragma unroll
      for (int k = 0; k < 8; ++k) col[k] = st[ST_ROW(k) + r];
      t = st[ST_DT];
      g = st[o_g];
      if constexpr (WARM) {
        const real* kn = L.kn(0);
#pragma unroll
        for (int k = 0; k < 8; ++k) pl[k] = kn[KN_R0 + k];
        pv = kn[KN_R0 + 8 + (r & 1)];
      }
    }
    const int in = N > 2 ? 1 : 0;
    unsigned a_nxt = lds_addr(L.st(in) + r);                                 // column-indexed: M(r, :) of the stage fetched ahead
    unsigned a_ng = lds_addr(L.st(in) + o_g);                                // ... its g
    unsigned a_uni = lds_addr(L.st(in));                                     // ... and, wave-uniform, its dt
    unsigned a_pl = lds_addr(L.kn(in) + KN_R0);                              // WARM: the plan's knot of that stage (wave-uniform)
    unsigned a_pv = lds_addr(L.kn(in) + KN_R0 + 8 + (r & 1));
    unsigned a_z = lds_addr(own ? L.kn(1) + r : junk0);                      // store targets (a dead cell: stride 0)
    unsigned a_v = lds_addr((own && r >= 6) ? L.kn(0) + 2 + r : junk1);
    const unsigned s_z = own ? kb : 0u, s_v = (own && r >= 6) ? kb : 0u;
    for (int i = 0; i < N - 1; ++i) {
      CHAIN_ADDR_PIN(a_nxt); CHAIN_ADDR_PIN(a_ng); CHAIN_ADDR_PIN(a_uni); CHAIN_ADDR_PIN(a_z); CHAIN_ADDR_PIN(a_v);
      if constexpr (WARM) { CHAIN_ADDR_PIN16(a_pl); CHAIN_ADDR_PIN(a_pv); }
      const LMPC_LDS real* const p_nxt = lds_at<real>(a_nxt);
      real dz[8];
      row_bcast8(d, dz);
      real acc = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) acc = rfma(col[k], dz[k], acc);
      const real ax = acc;
      acc = rfma(col[6], dz[6], acc);
      acc = rfma(col[7], dz[7], acc);
      real v = -acc;
      if constexpr (WARM) {  // (lanes 6, 7: col = a row of K)  v = v^plan + K z^plan - K z
        real kz = pv;
#pragma unroll
        for (int k = 0; k < 8; ++k) kz = rfma(col[k], pl[k], kz);
        v += kz;
      }
      const real u = rfma(t, v, d);  // (lanes 6, 7: their own component of z is u_{i-1})
      real u0, u1;
      row_bcast67(u, u0, u1);
      const real b0 = col[6], b1 = col[7], gi = g;
#pragma unroll
      for (int k = 0; k < 8; ++k) col[k] = p_nxt[ST_ROW(k)];
      t = lds_at<real>(a_uni)[ST_DT];
      g = *lds_at<real>(a_ng);
      if constexpr (WARM) {
#pragma unroll
        for (int k = 0; k < 8; ++k) pl[k] = lds_at<real>(a_pl)[k];
        pv = *lds_at<real>(a_pv);
      }
      const real nx = gi + rfma(b1, u1, rfma(b0, u0, ax));
      d = (r < 6) ? nx : u;
      *lds_at<real>(a_z) = d;
      *lds_at<real>(a_v) = v;
      const unsigned s_nxt = i < N - 3 ? sb : 0u;  // (the fetch ahead stops at the last stage)
      a_nxt += s_nxt; a_ng += s_nxt; a_uni += s_nxt; a_z += s_z; a_v += s_v;
      if constexpr (WARM) {
        const unsigned s_pl = i < N - 3 ? kb : 0u;
        a_pl += s_pl; a_pv += s_pl;
      }
    }
    wave_sync();
  } else {
    int nch = 0, cb = 0;
    if constexpr (SC::lean) {
      nch = (N - 2) / LN_CHUNK + 1;  // chunks of the model
      cb = r < 6 ? r : 0;
      MS.ensure(0);
      MS.wait();
      if (nch > 1) MS.ensure(1);
    }
    for (int i = 0; i < N - 1; ++i) {
      const real* st = L.st(i);
      const real* ab = SC::model(L, MS, i);
      real* kn = L.kn(i);
      real dz[8], col[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) dz[k] = kn[k];
      if constexpr (SC::lean) {  // (lanes r < 6: their row of [A B], stride 6 in the model record; lanes 6, 7: their row of K, stride 2 in the stage record)
#pragma unroll
        for (int k = 0; k < 8; ++k) col[k] = r < 6 ? ab[6 * k + cb] : st[2 * k + (r - 6)];
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) col[k] = st[SC::row(k) + r];
      }
      const real t = st[SC::dt];
      const real g = ab[SC::g + (SC::lean ? cb : (r < 6 ? r : 0))];
      real acc = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) acc = rfma(col[k], dz[k], acc);
      const real ax = acc;
      acc = rfma(col[6], dz[6], acc);
      acc = rfma(col[7], dz[7], acc);
      real v = -acc;
      if constexpr (WARM) {  // (lanes 6, 7: col = a row of K)  v = v^plan + K z^plan - K z
        real kz = kn[KN_R0 + 8 + (r & 1)];
#pragma unroll
        for (int k = 0; k < 8; ++k) kz = rfma(col[k], kn[KN_R0 + k], kz);
        v += kz;
      }
      const real u = rfma(t, v, (r == 6) ? dz[6] : dz[7]);
      const real u0 = lane_bcast(u, 6), u1 = lane_bcast(u, 7);
      const real nx = g + rfma(col[7], u1, rfma(col[6], u0, ax));
      *(own ? kn + LMPC_KNOT_STRIDE + r : junk0) = (r < 6) ? nx : u;
      *((own && r >= 6) ? kn + 2 + r : junk1) = v;
      wave_sync();
      if constexpr (SC::lean) if ((i % LN_CHUNK) == LN_CHUNK - 1 && i < N - 2) {  // the next stage is the first of the chunk above
        MS.wait();
        if (i / LN_CHUNK + 2 < nch) MS.fetch(i / LN_CHUNK + 2);
      }
    }
  }
}

// ======== the active-set polish (polish_limits, lmpc_limits.hip.h; the twin's polish() runs the same rounds) ========
// ONE body on the device, lmpc_polish<real, KQ, KS, io, TEAM>, for every kernel that polishes: the one-wave kernels (fp64, mixed, fp32,
// warm, second pass, tracking and learning: TEAM = Wave1, below) and the two-wave fp64 tracking kernels (TEAM = Wave2,
// lmpc_solve_w2.hip.h: KS = 0, real = io = double).  The twin is the only mirror of its rules.  In the profiling build
// (LMPC_PHASE_TIMING) the two-wave instances now keep the polish's own clocks as well and hand them back in PolishResult::prof; their
// caller does not add them to its buckets.  LMPC_POLISH_TRACE prints from thread 0 of workgroup 0 under either team.
// A CALL in the fp64 kernels (lmpc_polish_is_call, lmpc_solve_layout.hip.h), not part of the interior point's body (round 4; until then a lambda inlined into the solve): the polish keeps
// ~190 B more state per lane alive than an iteration does, and inlined -- even in an outer loop of its own -- it weighed on
// the register allocation of the iteration: 292 B of scratch per lane in the N = 20 fp64 kernel (824 B in the mixed learning
// kernel), 88 of the 116 scratch reloads of an iteration, +10 % per iteration.  Behind a call boundary the two are allocated
// separately.  What crosses it is passed BY VALUE (the iteration's arrays must not escape: an array whose address is taken
// lives in scratch for good): the row state t, lambda of the interior point (read only), the slot tables, the simplex rows,
// the wave-wide scalars.  The iterate itself is in LDS, which the callee names through the workgroup's dynamic LDS symbol
// (its accesses stay DS instructions).  Slacks and multipliers of the interior point are not touched; the iterate is put
// aside in the handle's save area and comes back unless the attempt is accepted.  Wave-uniform values arrive in vector
// registers (the calling convention has no scalar arguments) and go back to scalar registers first thing.
// Every instantiation runs the DPP form of the vector solves (riccati_solve_fat, riccati_solve_lean) since round 4: bit for bit the
// LDS-exchange forms of rounds 2-3, -3 % at N = 40 tracking / IAC, -8 % at N = 60, -4 % at N = 80, -4 / -12 % for the learning
// problem at N = 60 / 80.  (Rounds 2-3 kept DPP out of the one-wave-per-SIMD kernels after a non-reproducible KQ = 14 / KS = 3
// build; with the polish behind a call that family has been bit-stable in every build since.  The LDS-exchange functions and
// their -D switches were removed in round 5: scratch/r5/experiment_switches.patch.)

template <typename real, int KQ, int KS>
struct PolishArgs {
  void* keep;      // this problem's block of the save area
  const void* ws;  // lean layout: this problem's records in the linearisation workspace (ModelStream::ws)
  int N, S, has_sigma, have0, have1, pol_rounds;
  int max_rounds;  // repairs this attempt may spend (polish_limits::rounds; fewer for a warm start)
  real qsig, inv_m, sigma;
  int o_val[KQ], o_hl[KQ], s_gf[KQ];
  real s_tu[KQ], s_tl[KQ], s_lu[KQ], s_ll[KQ];
  SimplexRows<double, KS> sx;
};
template <typename real, int KS>
struct PolishResult {
  int accepted, pol_rounds, have0, have1;
  int noise;  // refused, and the last round failed on nothing but the multiplier steps / the held rows' residual (see the exit of lmpc_solve_problem)
  real sigma, mu, rdmax, last_step;
  double lm[KS > 0 ? KS : 1];  // the simplex weights of an accepted polish
#ifdef LMPC_PHASE_TIMING
  long long prof[4];  // the attempt's own clocks: factorisations, backward sweeps, forward sweeps, everything else
#endif
};

// ---- the team that runs the row phases of the interior point and of the polish ----
// lmpc_solve_problem and lmpc_polish below are each ONE body for one wave per problem and for two (lmpc_solve_w2.hip.h).  A team states
// what differs between the two, and nothing else -- none of it is arithmetic on a row:
//   THREADS, tid, lane    who owns the rows: a row loop is `for (e = tid; e < n; e += THREADS)`; lane is the lane within the wave, which
//                         deals the slots and is what the stage chains are written in
//   CHAIN                 whether this wave runs the stage chains; after_chain() is what shows the team a chain's results
//   SLOT0                 the first slot of this wave: slot j = SLOT0 + lane + 64 q
//   OPAQUE                whether a slot's table integers are read through an empty asm wherever a body reads one by itself (table();
//                         lmpc_solve_problem's SlotRef has the account)
//   CLASS, LEAN, FORM, PRIO   the kernel's class (the one-wave KQ, which bounds the horizon), its layout, the form of its stage chains and
//                         Lds::chain_prio: not of the slots per lane a body is instantiated with
//   attach(tail)          where the team exchanges, once the LDS block is known (the team itself is made first: the lane is read first)
//   sync()                the exchange of LDS content inside the team (the simplex blocks, one wave's, keep their wave_fence)
//   published()           behind an exchange that has to have published the LDS writes before it: two waves' exchange had a barrier
//   what the interior point alone asks (policies of the class, lmpc_solve_layout.hip.h, that the body once computed from its KQ):
//   LEARN                 whether the load honours P.learning
//   ROW_CHUNK             slots a row phase takes in one go (lmpc_row_chunk; two waves: all of a lane's)
//   OPAQUE_SLOTS, SITES   whether the row phases' SlotRef passes through the empty asm (lmpc_opaque_slots), and where it does otherwise
//                         (lmpc_opaque_sites)
//   FUSE                  the predictor's backward sweep inside the factorisation (lmpc_fuse_bwd)
//   NBHD                  whether the class has the wide-neighbourhood rule (fp64, KQ <= 7 of the CLASS)
//   POLISH_CALL, polish_call(a)   whether the polish is a call, and the call
//   uniform(x)            a scalar the team has agreed on, where the iteration carries it on: one wave moves it to scalar registers (uni),
//                         two waves leave it where it is -- their exchange has already done so, and uni is opaque to the optimiser
//   publish(next)         after the primal update: publishes it, unless an exchange follows (`next`) whose barrier does
//   after_polish()        what brings the team together again behind a polish attempt
//   sum2(v), max(x), min(x), all(p)   the team's sums of two values at once, maximum, minimum, and whether p holds on every lane
//   exchanged(x), sum_of(x)   the sacc sum in two steps, as step_end / max_of in the polish: two waves exchange once ahead of the pass's two
//                         arms and sum_of answers from it, one wave does nothing there and reduces in the arm that reads it
//   ROUNDED_CSIG          whether the rows phase forms the coupling cell's address in o_csig(q), which keeps `thd - thu` a rounded difference
//                         (the store has the account: it is about the bits the two-wave kernels have always returned, not about tables)
//   and one operation per exchange point of the bodies, each of them what the body did there before it had a team:
//   weights_sum(q, x)     q + the team's sum of x (the weights' eysum)
//   sum3(v)               three sums at once (the Schur step)
//   step_end(step, nan)   the end of a multiplier step: the largest step, and whether any lane's step was not finite
//   kkt(..)               the KKT exchange: four votes, the most negative multiplier, the worst row
//   any_of / min_of / max_of (slot, x)   what step_end and kkt agreed on, read at the point of use by its PolishSlot and with the lane's
//                         own value: one wave reduces THERE and step_end / kkt do nothing (a DPP reduction is not sunk by the compiler:
//                         the minimum is taken only after the acceptance test, the maximum only inside it; the ballots are behind the
//                         short-circuits they were behind), two waves have agreed on all of it in the one exchange and answer from it
//   mean(x, inv_m)        inv_m * the team's sum of x (the complementarity of an accepted point)
//   changed(p)            whether p holds on any lane (did a repair change the held set)
//   sum(x)                the team's sum (LMPC_POLISH_TRACE only)
// Every result is the same bits in every lane of the team, so the team takes every branch together.
// The operations pass plain values and return plain values: an aggregate returned or a result written through a reference changed the
// one-wave kernels' device code (the order of two scalar moves in <double, 4, 0, double>, more in the fp32 kernels), and so did reading
// the lane after N (scratch/isa_diff.py).
enum PolishSlot { PS_STEP = 0, PS_NAN = 1, PK_BAD = 0, PK_NEG = 1, PK_WEAK = 2, PK_VIOL = 3, PK_YMIN = 4, PK_WORST = 5 };

template <typename real, int KQ, int KS, typename io, bool SECOND = false>
__device__ PolishResult<real, KS> lmpc_polish_call(const PolishArgs<real, KQ, KS> a);  // (behind the polish)

template <int REAL_BYTES, int KQ, int KS, bool SECOND>
struct Wave1 {
  static constexpr int THREADS = 64, SLOT0 = 0, CLASS = KQ;
  static constexpr bool CHAIN = true, OPAQUE = false, ROUNDED_CSIG = false;
  static constexpr bool LEAN = lmpc_lean(REAL_BYTES, KQ);
  static constexpr ChainForm FORM = lmpc_chain_form(LEAN, lmpc_chain_addr(REAL_BYTES, KQ, KS));
  static constexpr bool PRIO = !SECOND && lmpc_waves_per_simd(REAL_BYTES, KQ, KS) >= 2;
  static constexpr bool LEARN = true;
  static constexpr int ROW_CHUNK = lmpc_row_chunk(REAL_BYTES, KQ, KS), SITES = lmpc_opaque_sites(REAL_BYTES, KQ, KS);
  static constexpr bool OPAQUE_SLOTS = lmpc_opaque_slots(REAL_BYTES, KQ, KS), FUSE = lmpc_fuse_bwd(REAL_BYTES, KQ, KS);
  static constexpr bool NBHD = REAL_BYTES == 8 && KQ <= 7, POLISH_CALL = lmpc_polish_is_call(REAL_BYTES, KQ, KS);
  static constexpr bool RID = lmpc_reduce_identity(REAL_BYTES, KQ, KS, 1);  // (the DPP reductions keep their identity operand)
  const int tid, lane;
  __device__ __forceinline__ Wave1() : tid(threadIdx.x), lane(threadIdx.x) {}
  template <typename real>
  __device__ static __forceinline__ void attach(real*) {}  // (tail of the LDS block: where two waves exchange)
  __device__ static __forceinline__ int table(int v) { return v; }
  __device__ static __forceinline__ void sync() { wave_sync(); }
  __device__ static __forceinline__ void published() { wave_sync(); }
  __device__ static __forceinline__ void after_chain() {}
  template <typename real>
  __device__ static __forceinline__ real uniform(real x) { return uni(x); }
  template <typename real>
  __device__ static __forceinline__ real exchanged(real x) { return x; }
  template <typename real>
  __device__ static __forceinline__ real sum_of(real x) { return wave_sum<RID>(x); }
  __device__ static __forceinline__ void publish(bool) { wave_sync(); }
  __device__ static __forceinline__ void after_polish() {}
  template <typename real, typename io>  // (the function itself, not a wrapper of it: what crosses the call stays by value as the caller wrote it)
  static constexpr PolishResult<real, KS> (*polish_call)(const PolishArgs<real, KQ, KS>) = &lmpc_polish_call<real, KQ, KS, io, SECOND>;
  template <typename real>
  __device__ static __forceinline__ void sum2(real (&v)[2]) { wave_sum_n<2, RID>(v); }
  template <typename real>
  __device__ static __forceinline__ real max(real x) { return wave_max<RID>(x); }
  template <typename real>
  __device__ static __forceinline__ real min(real x) { return wave_min<RID>(x); }
  __device__ static __forceinline__ bool all(bool p) { return wave_min<RID>(p ? 1.0 : 0.0) > 0.5; }
  template <typename real>
  __device__ static __forceinline__ real weights_sum(real q, real x) { return uni(q + wave_sum<RID>(x)); }
  template <typename real>
  __device__ static __forceinline__ void sum3(real (&v)[3]) { wave_sum_n<3, RID>(v); }
  template <typename real>
  __device__ static __forceinline__ void step_end(real, bool) {}  // (nothing yet: every value is reduced where it is read)
  template <typename real>
  __device__ static __forceinline__ void kkt(bool, bool, bool, bool, real, real) {}
  __device__ static __forceinline__ bool any_of(int, bool p) { return __ballot(p) != 0; }
  template <typename real>
  __device__ static __forceinline__ real min_of(int, real x) { return wave_min<RID>(x); }
  template <typename real>
  __device__ static __forceinline__ real max_of(int, real x) { return wave_max<RID>(x); }
  template <typename real>
  __device__ static __forceinline__ real mean(real x, real inv_m) { return uni(wave_sum<RID>(x) * inv_m); }
  __device__ static __forceinline__ bool changed(bool p) { return __ballot(p) != 0; }
  template <typename real>
  __device__ static __forceinline__ real sum(real x) { return wave_sum<RID>(x); }
};

// KQ: slots per lane (one wave: the class's; two waves: lmpc_w2_slots of it, and the class is the team's)
template <typename real, int KQ, int KS, typename io, class TEAM>
__device__ __forceinline__ PolishResult<real, KS> lmpc_polish(const PolishArgs<real, KQ, KS>& a) {
  static_assert(KS == 0 || TEAM::THREADS == 64, "the simplex rows and the terminal block are one wave's");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  real* const lds = reinterpret_cast<real*>(lds_raw);
  typedef typename vec2<real>::type real2;
  typedef double treal;
  typedef polish_limits<real> pol;
  TEAM tm;
  const int tid = tm.tid, lane = tm.lane;
  const int N = uni(a.N), NS = N - 1;
  constexpr bool LEAN = TEAM::LEAN;
  constexpr ChainForm FORM = TEAM::FORM;
  Lds<real> L{lds, N, LEAN ? LMPC_LEAN_STAGE_STRIDE : LMPC_STAGE_STRIDE, TEAM::PRIO};
  real* const T = L.tail();
  tm.attach(T);
  treal* const TT = reinterpret_cast<treal*>(T + LMPC_TAIL_DOUBLES);
  ModelStream<real> MS{nullptr, nullptr, NS, lane, uni(a.have0), uni(a.have1)};
  if constexpr (LEAN) {
    MS.ws = uni_ptr(reinterpret_cast<const real*>(a.ws));
    MS.buf = reinterpret_cast<real*>(reinterpret_cast<unsigned char*>(TT) +
                                     (KS > 0 ? (LMPC_TERM_CELLS + 6 * LMPC_SS_STRIDE(uni(a.S))) * sizeof(treal) : 0));
  }
  const real inf = real(INFINITY);
  const treal tinf = treal(INFINITY);
  const bool has_sigma = uni(a.has_sigma) != 0;
  const real qsig = uni(a.qsig), inv_m = uni(a.inv_m);
  real sigma = uni(a.sigma);
  real hsig = 0.0, ce = 0.0, mu = 0.0, rdmax = 0.0, last_step = 0.0;
  int pol_rounds = uni(a.pol_rounds);
  PT_DECL
  (void)pf;
  (void)tinf;
  const int KNB = NS * L.stride;
  const int JB = KNB + N * LMPC_KNOT_STRIDE + TL_W;
  const int CTB = KNB + N * LMPC_KNOT_STRIDE + TL_CT;
  int o_val[KQ], o_hl[KQ], s_gf[KQ];
  real s_tu[KQ], s_tl[KQ], s_lu[KQ], s_ll[KQ], s_pu[KQ], s_pl[KQ];
#pragma unroll
  for (int q = 0; q < KQ; ++q) {
    o_val[q] = a.o_val[q];
    o_hl[q] = a.o_hl[q];
    s_gf[q] = a.s_gf[q];
    s_tu[q] = a.s_tu[q];
    s_tl[q] = a.s_tl[q];
    s_lu[q] = a.s_lu[q];
    s_ll[q] = a.s_ll[q];
    s_pu[q] = s_pl[q] = 0.0;
  }
  SimplexRows<treal, KS> sx = a.sx;
  if constexpr (KS > 0) {
    sx.ul = TT + TL_UL;
    sx.tau = uni(sx.tau);
#pragma unroll
    for (int k = 0; k < 6; ++k) sx.ss0[k] = uni(sx.ss0[k]);
  }
  auto ovq = [&](int q) { return TEAM::table(o_val[q]); };  // (the slot's table integers as the row phases read them)
  auto ohq = [&](int q) { return TEAM::table(o_hl[q]); };
  auto gfq = [&](int q) { return TEAM::table(s_gf[q]); };
  auto flags = [&](int q) { return gfq(q) >> 20; };
  auto o_w = [&](int q) { return ovq(q) + ((flags(q) & F_EY) ? KN_EY - 1 : KN_R0); };
  auto o_csig = [&](int q) { return (flags(q) & F_EY) ? ovq(q) + (KN_CSIG - 1) : JB + KN_CSIG; };
  auto bounds = [&](int q) { return *reinterpret_cast<const real2*>(&lds[ohq(q)]); };
  // The iterate is put aside in the handle's save area -- one contiguous block of 10 N - 4 values per problem (full-line
  // writes), values as they stand in LDS, so that they read back exactly -- and taken back from there at the start of every
  // round and when the attempt is refused: every lane reads back what it wrote itself.
  io* const keep = uni_ptr(reinterpret_cast<io*>(a.keep));
  auto put_keep = [&]() {
    for (int e = tid; e < 10 * N - 4; e += TEAM::THREADS) {  // knot i: z [8] (x_i, u_{i-1}) at 10 i - 2 .. (knot 0: x_0 only is not kept), v_i [2] behind it
      const int i = (e + 2) / 10, o = e + 2 - 10 * i;
      keep[e] = io(L.kn(i)[o]);
    }
  };
  auto get_primal = [&]() {
    for (int e = tid; e < 10 * N - 4; e += TEAM::THREADS) {
      const int i = (e + 2) / 10, o = e + 2 - 10 * i;
      if (i >= 1 || o >= 8) L.kn(i)[o] = real(keep[e]);
    }
  };
  // (bit 8 of max_rounds: the attempt at the interior point's EXIT, fp64: in doubt -- lam ~ t, a weakly active row -- a row is held,
  //  from lam > 1e-2 t on; held wrongly it comes out with a negative multiplier and the next round releases it, free wrongly it is
  //  violated, drags its neighbours' multipliers below zero and the repairs release THEM.  oracle/c/lmpc_oracle.c, POLISH_EXIT, has
  //  the problem this was found on.)
  const real gam = (sizeof(real) == 8 && (uni(a.max_rounds) & POLISH_EXIT)) ? real(POLISH_EXIT_GAMMA) : real(1);
  int held = 0;  // (per lane) bit 2q / 2q + 1: upper / lower row of slot q held; bit 28 + q: simplex row q held
#pragma unroll
  for (int q = 0; q < KQ; ++q) held |= (s_lu[q] > gam * s_tu[q] ? 1 << (2 * q) : 0) | (s_ll[q] > gam * s_tl[q] ? 2 << (2 * q) : 0);
  if constexpr (KS > 0) {
#pragma unroll
    for (int q = 0; q < KS; ++q) {
      held |= (sx.on[q] && sx.l[q] > sx.t[q]) ? 1 << (28 + q) : 0;
      sx.sv[q] = sx.lm[q];
    }
  }
  const real sigma_keep = sigma;
  put_keep();
  bool accepted = false, noise = false;
  const int max_rounds = min((int)pol::rounds, uni(a.max_rounds) & ~POLISH_EXIT);
  for (int round = 0; round < max_rounds; ++round) {
    if (round > 0) {  // every round starts from the interior point's iterate
      tm.sync();
      get_primal();
      sigma = sigma_keep;
      if constexpr (KS > 0) {
#pragma unroll
        for (int q = 0; q < KS; ++q) sx.lm[q] = sx.sv[q];
      }
      tm.sync();
    }
    // ---- weights: theta on the held rows, nothing on the others; multipliers start from the interior point's on the
    // rows it held itself and from zero on rows a repair has added ----
    real eysum = 0.0;
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
      const int f = flags(q);
      const bool hu = (held >> (2 * q)) & 1, hd = (held >> (2 * q + 1)) & 1;
      const real thu = hu ? real(pol::theta) : real(0), thd = hd ? real(pol::theta) : real(0);
      lds[o_w(q)] = thu + thd;
      lds[o_csig(q)] = (f & F_SIG) ? (thd - thu) : real(0);
      eysum += (f & F_SIG) ? (thu + thd) : real(0);
      s_pu[q] = (hu && s_lu[q] > s_tu[q]) ? s_lu[q] : real(0);
      s_pl[q] = (hd && s_ll[q] > s_tl[q]) ? s_ll[q] : real(0);
    }
    if constexpr (KS > 0) {
      // the free simplex weights have theta = 0 and must ALL be explicit unknowns of the terminal block: more than MA_MAX
      // of them and the round cannot be set up
      treal thq[KS];
      int nfree = 0;
#pragma unroll
      for (int q = 0; q < KS; ++q) {
        const bool hq = (held >> (28 + q)) & 1;
        thq[q] = !sx.on[q] ? tinf : (hq ? treal(POLISH_THETA_L) : treal(0));
        sx.aidx[q] = -1;
        nfree += (sx.on[q] && !hq) ? 1 : 0;
        sx.p[q] = (hq && sx.l[q] > sx.t[q]) ? sx.l[q] : treal(0);
      }
      if (__popcll(__ballot(nfree > 0)) + __popcll(__ballot(nfree > 1)) + __popcll(__ballot(nfree > 2)) > MA_MAX) break;
      if (lane < 6 * MA_MAX) TT[TL_UA + lane] = 0.0;
      if (lane < MA_MAX) {
        TT[TL_THA + lane] = 1.0;
        TT[TL_RA + lane] = 0.0;
      }
      wave_fence();
      int m = 0;
      for (int a = 0; a < MA_MAX; ++a) {
        treal cand = tinf;
        int cq = 0;
#pragma unroll
        for (int q = 0; q < KS; ++q) {
          const bool better = sx.aidx[q] < 0 && thq[q] < sx.tau && thq[q] < cand;
          cand = better ? thq[q] : cand;
          cq = better ? q : cq;
        }
        const treal best = wave_min<TEAM::RID>(cand);
        if (!(best < tinf)) break;
        const int owner = __ffsll((long long)__ballot(cand == best)) - 1;
        if (lane == owner) {
#pragma unroll
          for (int q = 0; q < KS; ++q)
            if (q == cq) {
              sx.aidx[q] = a;
              treal uq[6];
              sx.load_u(q, lane, uq);
#pragma unroll
              for (int k = 0; k < 6; ++k) TT[TL_UA + a * 6 + k] = uq[k];
              TT[TL_THA + a] = thq[q];
            }
        }
        wave_fence();
        m = a + 1;
      }
      sx.m = m;
      wave_fence();
      treal tt[21], av[14];
#pragma unroll
      for (int k = 0; k < 21; ++k) tt[k] = 0.0;
#pragma unroll
      for (int k = 0; k < 14; ++k) av[k] = 0.0;
#pragma unroll
      for (int q = 0; q < KS; ++q) {
        const treal itf = (sx.on[q] && sx.aidx[q] < 0) ? frcp(thq[q]) : treal(0);
        int n = 0;
        treal uq[6];
        sx.load_u(q, lane, uq);
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
          for (int c = r; c < 6; ++c) tt[n++] += uq[r] * uq[c] * itf;
          av[r] += uq[r] * itf;
          av[7 + r] += uq[r] * sx.lm[q];
        }
        av[6] += itf;
        av[13] += sx.lm[q];
      }
      {
        treal red[32], red3[3] = {av[11], av[12], av[13]};
#pragma unroll
        for (int k = 0; k < 21; ++k) red[k] = tt[k];
#pragma unroll
        for (int k = 0; k < 11; ++k) red[21 + k] = av[k];
        wave_sum_split<32, TEAM::RID>(red, lane);
        wave_sum_split<3, TEAM::RID>(red3, lane);
#pragma unroll
        for (int k = 0; k < 21; ++k) tt[k] = red[k];
#pragma unroll
        for (int k = 0; k < 11; ++k) av[k] = red[21 + k];
        av[11] = red3[0];
        av[12] = red3[1];
        av[13] = red3[2];
      }
      sx.r1 = 1.0 - av[13];
      {
        treal F[36], aB[6];
        int n = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
          for (int c = r; c < 6; ++c) {
            F[r * 6 + c] = tt[n];
            F[c * 6 + r] = tt[n];
            ++n;
          }
          aB[r] = av[r];
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) F[k * 6 + k] += 1.0 / fmax(TT[TL_E + k], treal(1e-30));
        term_factor_u(TT, lane, F, aB, av[6], m);
      }
      if (lane < 6) {
        treal e = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k)
          if (k == lane) e = (treal(L.kn(N - 1)[k]) - sx.ss0[k]) - av[7 + k];
        TT[TL_EPS + lane] = e;
      }
      wave_fence();
    }
    hsig = tm.weights_sum(qsig, eysum);
    ++pol_rounds;
    tm.published();  // (the weights)
    PT_MARK(0)
    if constexpr (TEAM::CHAIN) riccati_factor<FORM, (KS > 0), true>(L, MS, lane, TT + TL_PT);
    tm.after_chain();
    PT_MARK(3)
    bool nan_step = false;
    // ---- pol::steps multiplier steps on that factor, each from the point the one before has reached ----
    for (int k = 0; k < pol::steps; ++k) {
      treal eeps[6] = {0, 0, 0, 0, 0, 0};
      if constexpr (KS > 0) {
#pragma unroll
        for (int c = 0; c < 6; ++c) eeps[c] = uni(TT[TL_E + c] * TT[TL_EPS + c]);
        treal bs[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < KS; ++q) {
          treal itf, uq[6];
          sx.load_u(q, lane, uq);
          const treal rj = sx.on[q] ? -simplex_bl_polish(sx.lm[q], sx.p[q], ((held >> (28 + q)) & 1) != 0, sx.j[q], uq, eeps, itf) : treal(0);
          if (sx.aidx[q] >= 0) TT[TL_RA + sx.aidx[q]] = rj;
          const treal w = (sx.on[q] && sx.aidx[q] < 0) ? rj * itf : treal(0);
          bs[6] += w;
#pragma unroll
          for (int c = 0; c < 6; ++c) bs[c] += uq[c] * w;
        }
        wave_sum_split<7, TEAM::RID>(bs, lane);
        wave_fence();
        treal beta[6], h[6], nu;
#pragma unroll
        for (int c = 0; c < 6; ++c) beta[c] = bs[c];
        term_solve_u(TT, lane, sx.m, beta, bs[6], sx.r1, h, nu);
        if (lane < 6) {
          treal hs = h[0];
#pragma unroll
          for (int c = 1; c < 6; ++c) hs = (lane == c) ? h[c] : hs;
          TT[TL_TG + lane] = TT[TL_E + lane] * TT[TL_EPS + lane] - hs;
        }
        wave_fence();
      }
      real sgsum = 0.0;
      {  // gradient: cost gradient + (y + theta * residual) on the held rows
        real val[KQ], par[KQ], ca[KQ], cb[KQ], ql[KQ];
        real2 hl[KQ];
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
          const int gr = gfq(q);
          val[q] = lds[ovq(q)];
          hl[q] = bounds(q);
          par[q] = lds[ovq(q) + ((gr >> 16) & 3) - 1];
          ca[q] = lds[CTB + (gr & 0xff)];
          cb[q] = lds[CTB + ((gr >> 8) & 0xff)];
          ql[q] = lds[ovq(q) + (KN_QLIN - 3)];
        }
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
          const int f = flags(q);
          const real sg = (f & F_SIG) ? sigma : 0.0;
          const bool hu = (held >> (2 * q)) & 1, hd = (held >> (2 * q + 1)) & 1;
          const real cu = hu ? rfma(real(pol::theta), val[q] - sg - hl[q].x, s_pu[q]) : real(0);
          const real cd = hd ? rfma(real(pol::theta), -val[q] - sg + hl[q].y, s_pl[q]) : real(0);
          const real gq = ca[q] * val[q] + cb[q] * par[q] + ((f & F_QLIN) ? ql[q] : real(0));
          lds[o_w(q)] = gq + cu - cd;
          if (k == 0) lds[(f & F_EY) ? JB + KN_EY : o_w(q) + 10] = 0.0;
          sgsum += (f & F_SIG) ? (cu + cd) : real(0);
        }
      }
      tm.sync();
      for (int i = tid; i < N; i += TEAM::THREADS) {
        real* kn = L.kn(i);
        kn[KN_R0 + 1] += kn[KN_EY];
        if (k == 0) kn[KN_R1 + 1] = (i >= 1) ? kn[KN_CSIG] : 0.0;
      }
      if constexpr (KS > 0) {
        wave_sync();
        if (lane < 6) L.kn(N - 1)[KN_R0 + lane] += real(TT[TL_TG + lane]);
      }
      tm.sync();
      PT_MARK(0)
      if constexpr (TEAM::CHAIN) {
        if (k == 0 && has_sigma)
          riccati_solve<FORM, 2>(L, MS, lane, pf);
        else
          riccati_solve<FORM, 1>(L, MS, lane, pf);
      }
      tm.after_chain();
      real dz0[KQ], dz1[KQ], val[KQ];
      real2 hl[KQ];
#pragma unroll
      for (int q = 0; q < KQ; ++q) {
        dz0[q] = lds[ovq(q) + 10];
        dz1[q] = lds[ovq(q) + 20];
        val[q] = lds[ovq(q)];
        hl[q] = bounds(q);
      }
      real dsigma = 0.0;
      if (has_sigma) {
        real red[3] = {0.0, 0.0, sgsum};
        {
          real cs[KQ];
#pragma unroll
          for (int q = 0; q < KQ; ++q) cs[q] = lds[o_csig(q)];
#pragma unroll
          for (int q = 0; q < KQ; ++q) {
            const bool sch = (flags(q) & F_SCH) != 0;
            red[0] += sch ? cs[q] * dz0[q] : real(0);
            red[1] += sch ? cs[q] * dz1[q] : real(0);
          }
        }
        tm.sum3(red);
        if (k == 0) ce = red[1];
        const real qsg = qsig * sigma - red[2];
        dsigma = uni(-(qsg + red[0]) / (hsig + ce));
      }
      if constexpr (KS > 0) {
        const real* knT = L.kn(N - 1);
        treal e[6], gs[7] = {0, 0, 0, 0, 0, 0, 0}, rj[KS], itfq[KS];
#pragma unroll
        for (int c = 0; c < 6; ++c) e[c] = TT[TL_E + c] * treal(knT[KN_R0 + c] + dsigma * knT[KN_R1 + c]);
#pragma unroll
        for (int q = 0; q < KS; ++q) {
          treal itf, uq[6];
          sx.load_u(q, lane, uq);
          treal r = -simplex_bl_polish(sx.lm[q], sx.p[q], ((held >> (28 + q)) & 1) != 0, sx.j[q], uq, eeps, itf);
#pragma unroll
          for (int c = 0; c < 6; ++c) r += uq[c] * e[c];
          r = sx.on[q] ? r : 0.0;
          rj[q] = r;
          itfq[q] = itf;
          if (sx.aidx[q] >= 0) TT[TL_RA + sx.aidx[q]] = r;
          const treal w = (sx.on[q] && sx.aidx[q] < 0) ? r * itf : treal(0);
          gs[6] += w;
#pragma unroll
          for (int c = 0; c < 6; ++c) gs[c] += uq[c] * w;
        }
        wave_sum_split<7, TEAM::RID>(gs, lane);
        wave_fence();
        treal beta[6], h[6], nu;
#pragma unroll
        for (int c = 0; c < 6; ++c) beta[c] = gs[c];
        term_solve_u(TT, lane, sx.m, beta, gs[6], sx.r1, h, nu);
#pragma unroll
        for (int q = 0; q < KS; ++q) {
          treal uh = 0.0, uq[6];
          sx.load_u(q, lane, uq);
#pragma unroll
          for (int c = 0; c < 6; ++c) uh += uq[c] * h[c];
          const treal dB = (rj[q] - nu - uh) * itfq[q];
          const treal dA = TT[TL_XA + (sx.aidx[q] >= 0 ? sx.aidx[q] : 0)];
          sx.dl[q] = sx.on[q] ? (sx.aidx[q] >= 0 ? dA : dB) : treal(0);
        }
      }
      // the full step, taken at once; multipliers from the residual BEFORE the step plus the row's own increment (the
      // stored value is rounded after the update, the increment is not: in single precision the re-read residual of a
      // row that has landed on its bound is exactly zero and says nothing)
      bool finite_step = dsigma == dsigma;
      real stepmax = 0.0;
#pragma unroll
      for (int q = 0; q < KQ; ++q) {
        const int f = flags(q);
        const real dval = dz0[q] + dsigma * dz1[q];
        finite_step = finite_step && (fabs(dval) < inf);
        stepmax = fmax(stepmax, (f & F_MOVE) ? fabs(dval) * real(slot_inv_scale((gfq(q) >> 27) & 15)) : real(0));
        const real sg = (f & F_SIG) ? sigma : 0.0, dsg = (f & F_SIG) ? dsigma : 0.0;
        const bool hu = (held >> (2 * q)) & 1, hd = (held >> (2 * q + 1)) & 1;
        s_pu[q] = hu ? rfma(real(pol::theta), (val[q] - sg - hl[q].x) + (dval - dsg), s_pu[q]) : real(0);
        s_pl[q] = hd ? rfma(real(pol::theta), (-val[q] - sg + hl[q].y) + (-dval - dsg), s_pl[q]) : real(0);
        const bool mv = (f & F_MOVE) != 0;
        lds[mv ? ovq(q) : JB + q] += mv ? dval : real(0);
      }
      if (has_sigma) sigma = uni(sigma + dsigma);
      if constexpr (KS > 0) {
#pragma unroll
        for (int q = 0; q < KS; ++q) {
          const bool hq = (held >> (28 + q)) & 1;
          sx.p[q] = hq ? sx.p[q] + treal(POLISH_THETA_L) * (-sx.lm[q] - sx.dl[q]) : treal(0);
          sx.lm[q] += sx.dl[q];
          finite_step = finite_step && (fabs(sx.dl[q]) < tinf);
        }
      }
      tm.step_end(stepmax, !finite_step);
      nan_step = nan_step || tm.any_of(PS_NAN, !finite_step);
      last_step = tm.max_of(PS_STEP, stepmax);  // (scaled: what kkt[0] reports after an accepted polish)
      tm.published();  // (the update)
      if constexpr (KS > 0) {  // the hull residual and the simplex residual at the new point (the next step's gradient)
        treal ul[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < KS; ++q) {
          treal uq[6];
          sx.load_u(q, lane, uq);
#pragma unroll
          for (int c = 0; c < 6; ++c) ul[c] += uq[c] * sx.lm[q];
          ul[6] += sx.lm[q];
        }
        wave_sum_split<7, TEAM::RID>(ul, lane);
        sx.r1 = 1.0 - ul[6];
        if (lane < 6) {
          treal e = 0.0;
#pragma unroll
          for (int c = 0; c < 6; ++c)
            if (c == lane) e = (treal(L.kn(N - 1)[c]) - sx.ss0[c]) - ul[c];
          TT[TL_EPS + lane] = e;
        }
        wave_fence();
      }
#ifdef LMPC_POLISH_TRACE
      if (blockIdx.x == 0 && tid == 0) printf("      step %d: %.3e\n", k, (double)last_step);
#endif
      if (k >= 1 && last_step <= real(pol::step_ok)) break;  // (converged: the remaining steps would move nothing)
    }
    // ---- KKT test of the point reached; repair of the held set ----
    real val[KQ];
    real2 hl[KQ];
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
      val[q] = lds[ovq(q)];
      hl[q] = bounds(q);
    }
    bool bad = false, neg = false, weakneg = false, viol = false;
    real ymin = 0.0, comp = 0.0, worst = 0.0;
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
      const int f = flags(q);
      const real sg = (f & F_SIG) ? sigma : 0.0;
      const real ru = val[q] - sg - hl[q].x, rl = -val[q] - sg + hl[q].y;
      const bool hu = (held >> (2 * q)) & 1, hd = (held >> (2 * q + 1)) & 1;
      const bool nu_ = hu && s_pu[q] < -real(pol::dual), nd_ = hd && s_pl[q] < -real(pol::dual);
      bad = bad || (hu && !(fabs(ru) <= real(pol::feas))) || (hd && !(fabs(rl) <= real(pol::feas)));
      neg = neg || nu_ || nd_;
      weakneg = weakneg || (nu_ && s_lu[q] < real(POLISH_STRONG) * s_tu[q]) || (nd_ && s_ll[q] < real(POLISH_STRONG) * s_tl[q]);
      viol = viol || (!hu && (f & F_UP) && !(ru <= real(pol::feas))) || (!hd && (f & F_LO) && !(rl <= real(pol::feas)));
      ymin = fmin(ymin, fmin(hu ? s_pu[q] : real(0), hd ? s_pl[q] : real(0)));
      comp += (hu ? fabs(s_pu[q] * ru) : real(0)) + (hd ? fabs(s_pl[q] * rl) : real(0));
      worst = fmax(worst, fmax((f & F_UP) ? ru : real(0), (f & F_LO) ? rl : real(0)));
    }
    if constexpr (KS > 0) {
#pragma unroll
      for (int q = 0; q < KS; ++q) {
        const bool hq = (held >> (28 + q)) & 1, fr = sx.on[q] && !hq;
        const bool nq = hq && sx.p[q] < -treal(pol::dual_l);
        bad = bad || (hq && !(fabs(sx.lm[q]) <= treal(pol::feas)));
        neg = neg || nq;
        weakneg = weakneg || (nq && sx.l[q] < treal(POLISH_STRONG) * sx.t[q]);
        viol = viol || (fr && !(-sx.lm[q] <= treal(pol::feas)));
        ymin = fmin(ymin, hq ? real(sx.p[q]) : real(0));
        comp += hq ? real(fabs(sx.p[q] * sx.lm[q])) : real(0);
      }
    }
    // (a last multiplier step that still moved the iterate: the steps have not converged -- held rows that are stiff meet
    // their bounds long before the point is stationary, so the row tests alone would pass)
    tm.kkt(bad, neg, weakneg, viol, ymin, worst);
    const bool anybad = nan_step || !(last_step <= real(pol::step_tol)) || tm.any_of(PK_BAD, bad);
    const bool anyneg = tm.any_of(PK_NEG, neg), anyweak = tm.any_of(PK_WEAK, weakneg);
    const bool anyviol = tm.any_of(PK_VIOL, viol);
#ifdef LMPC_POLISH_TRACE  // (diagnostics: workgroup 0 prints what each round's KKT test saw)
    {
      const real tr_held = tm.sum(real(__popc(held & 0x0fffffff))), tr_ymin = tm.min_of(PK_YMIN, ymin), tr_worst = tm.max_of(PK_WORST, worst);
      if (blockIdx.x == 0 && tid == 0)
        printf("polish round %d: held %d last_step %.3e bad %d (rows %d nan %d) neg %d weak %d viol %d ymin %.3e worst %.3e\n", pol_rounds, (int)tr_held,
               (double)last_step, (int)anybad, (int)tm.any_of(PK_BAD, bad), (int)nan_step, (int)anyneg, (int)anyweak, (int)anyviol, (double)tr_ymin, (double)tr_worst);
    }
#endif
    if (!anybad && !anyneg && !anyviol) {  // the optimum for the held set, and the held set passes the KKT test
      mu = tm.mean(comp, inv_m);
      rdmax = tm.max_of(PK_WORST, worst);
      accepted = true;
      break;
    }
    noise = anybad && !anyneg && !anyviol;  // a consistent held set whose multiplier steps did not converge
    // repair: release rows with a negative multiplier -- those the interior point did not hold firmly if there are such,
    // otherwise the most negative ones (a wrong row drags its neighbours' multipliers below zero) -- and only when no
    // multiplier is negative, hold the rows the new point violates
    const real ycut = real(0.5) * tm.min_of(PK_YMIN, ymin);
    const int before = held;
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
      const int f = flags(q);
      const real sg = (f & F_SIG) ? sigma : 0.0;
      const real ru = val[q] - sg - hl[q].x, rl = -val[q] - sg + hl[q].y;
      const bool hu = (held >> (2 * q)) & 1, hd = (held >> (2 * q + 1)) & 1;
      const bool du = hu && s_pu[q] < -real(pol::dual) && (anyweak ? s_lu[q] < real(POLISH_STRONG) * s_tu[q] : s_pu[q] <= ycut);
      const bool dd = hd && s_pl[q] < -real(pol::dual) && (anyweak ? s_ll[q] < real(POLISH_STRONG) * s_tl[q] : s_pl[q] <= ycut);
      const bool au = !anyneg && !hu && (f & F_UP) && !(ru <= real(pol::feas));
      const bool ad = !anyneg && !hd && (f & F_LO) && !(rl <= real(pol::feas));
      held = (held & ~((du ? 1 : 0) << (2 * q)) & ~((dd ? 2 : 0) << (2 * q))) | ((au ? 1 : 0) << (2 * q)) | ((ad ? 2 : 0) << (2 * q));
    }
    if constexpr (KS > 0) {
#pragma unroll
      for (int q = 0; q < KS; ++q) {
        const bool hq = (held >> (28 + q)) & 1, fr = sx.on[q] && !hq;
        const bool dq = hq && sx.p[q] < -treal(pol::dual_l) && (anyweak ? sx.l[q] < treal(POLISH_STRONG) * sx.t[q] : real(sx.p[q]) <= ycut);
        const bool aq = !anyneg && fr && !(-sx.lm[q] <= treal(pol::feas));
        held = (held & ~((dq ? 1 : 0) << (28 + q))) | ((aq ? 1 : 0) << (28 + q));
      }
    }
    if (!tm.changed(held != before)) break;  // (the multiplier steps did not converge on a consistent set: nothing to repair)
  }
  if (!accepted) {  // refused: iterate, slack variable and simplex weights as the interior point left them
    tm.sync();
    get_primal();
    sigma = sigma_keep;
    if constexpr (KS > 0) {
#pragma unroll
      for (int q = 0; q < KS; ++q) sx.lm[q] = sx.sv[q];
    }
    tm.sync();
  }
  PolishResult<real, KS> res;
  res.accepted = accepted ? 1 : 0;
  res.noise = (!accepted && noise) ? 1 : 0;
  res.pol_rounds = pol_rounds;
  res.have0 = MS.have0;
  res.have1 = MS.have1;
  res.sigma = sigma;
  res.mu = mu;
  res.rdmax = rdmax;
  res.last_step = last_step;
  if constexpr (KS > 0) {
#pragma unroll
    for (int q = 0; q < KS; ++q) res.lm[q] = sx.lm[q];
  }
#ifdef LMPC_PHASE_TIMING
  PT_MARK(0)
  res.prof[0] = pf.acc[3];
  res.prof[1] = pf.acc[8] + pf.acc[9];
  res.prof[2] = pf.acc[10] + pf.acc[11];
  res.prof[3] = pf.acc[0];
#endif
  return res;
}

template <typename real, int KQ, int KS, typename io, bool SECOND>
__device__ __attribute__((noinline)) PolishResult<real, KS> lmpc_polish_call(const PolishArgs<real, KQ, KS> a) {
  return lmpc_polish<real, KQ, KS, io, Wave1<sizeof(real), KQ, KS, SECOND>>(a);
}

// `real` is the arithmetic and LDS type, `io` the type of the arrays in HBM: <double, double> is the reference's
// precision, <float, float> the single-precision path, <float, double> the mixed path (fp64 linearisation, regression,
// safe-set centring and results around an fp32 interior-point iteration).
// One problem, solved by the calling team in the LDS block it is given: the body of every solve kernel, the one-wave kernels below
// (TEAM = Wave1) and the two-wave kernel of lmpc_solve_w2.hip.h (TEAM = Wave2: each of its waves runs this body on its half of the slots).
// KQ: slots per lane (one wave: the class's; two waves: lmpc_w2_slots of it, and the class is the team's).

// SECOND: the fp64 second pass of a mixed solve -- a handful of problems a whole batch waits for, sharing the chip with the next batch's
// first pass: its waves run at the top issue priority throughout (and do not drop it between chains).
template <typename real, int KQ, int KS, typename io, bool SECOND = false, bool WARMK = false,  // (WARMK: the warm-start kernels, below)
          class TEAM = Wave1<sizeof(real), KQ, KS, SECOND>>
__device__ __forceinline__ void lmpc_solve_problem(
    const lmpc_params& P, const int B, const int b, unsigned char* lds_raw, const io* __restrict__ ws_lin,
    const io* __restrict__ x_ic, const io* __restrict__ u_ic, const io* __restrict__ T_ref, const io* __restrict__ bl,
    const io* __restrict__ br, const io* __restrict__ vref, const io* __restrict__ ss_x,
    const io* __restrict__ ss_j, io* __restrict__ lam_out, io* __restrict__ X_out,
    io* __restrict__ U_out, io* __restrict__ dU_out, int* __restrict__ status_out,
    int* __restrict__ iters_out, io* __restrict__ kkt_out) {
  static_assert(TEAM::THREADS == 64 || (KS == 0 && !WARMK && !SECOND && std::is_same<real, double>::value && std::is_same<io, double>::value),
                "the simplex rows, the warm start, the second pass and single precision are one wave's");
  real* const lds = reinterpret_cast<real*>(lds_raw);
  TEAM tm;
  const int tid = tm.tid, lane = tm.lane;
  const int N = P.N, NS = N - 1;
  typedef typename vec2<real>::type real2;
  typedef double treal;  // the safe-set block (simplex rows, terminal elimination) is always carried in fp64
  typedef ipm_limits<real> lim;
  const real inf = real(INFINITY), marg = real(P.marg), qsig = real(P.qsig), tol = lim::tol(P.tol);
  // single precision carries the abscissa relative to x_ic[0] (the QP is invariant to the shift: A(:, s) = e_s)
  const io s_shift = sizeof(real) == 4 ? x_ic[b] : io(0);
  constexpr bool LEAN = TEAM::LEAN;
  // slots a row phase loads, computes and stores in one go: all of them where the registers hold the temporaries of all KQ at
  // once; LMPC_ROW_CHUNK at a time in the long-horizon kernels (KQ >= 11: 11-14 slots x 7 operands on top of 12 doubles of row
  // state per slot do not fit 512 registers, and what the allocator spills is the row state)
  constexpr int QC = TEAM::ROW_CHUNK;
  constexpr int SITES = TEAM::SITES;
  // the predictor's backward sweep inside the factorisation (riccati_factor<.., FUSE>): the barrier weights then go to the rhs1 cells
  // and the predictor's gradient is assembled ahead of the factorisation.  Problems without the shared slack have one right-hand
  // side and keep the five-chain iteration (no shipped configuration: q_boundary > 0 everywhere).
  // (the warm-start kernels too: their cold path is this iteration -- except at two waves per SIMD, where the fused iteration is only
  //  trusted with the polish behind a call, lmpc_fuse_bwd's comment, and the warm kernels keep theirs inline)
  constexpr bool WARM_INLINE = WARMK && lmpc_waves_per_simd(sizeof(real), KQ, KS) >= 2;
  constexpr bool FUSEK = TEAM::FUSE && !WARM_INLINE;
  constexpr ChainForm FORM = TEAM::FORM;  // of the stage chains (lmpc_solve_layout.hip.h)
  const bool fuse = FUSEK && P.has_sigma != 0;
  Lds<real> L{lds, N, LEAN ? LMPC_LEAN_STAGE_STRIDE : LMPC_STAGE_STRIDE, TEAM::PRIO};
  if constexpr (SECOND && LMPC_CHAIN_PRIO) __builtin_amdgcn_s_setprio(3);
  real* T = L.tail();
  tm.attach(T);
  real* ct = T + TL_CT;
  real* KN0 = L.kn(0);
  // terminal region (learning only): treal cells behind the records; 16-byte aligned because every record size is even
  treal* const TT = reinterpret_cast<treal*>(T + LMPC_TAIL_DOUBLES);
  // lean layout: the chunk buffers sit behind everything else (records, tail, terminal region)
  ModelStream<real> MS{nullptr, nullptr, NS, lane, -1, -1};
  if constexpr (LEAN) {
    static_assert(!LEAN || (std::is_same<real, double>::value && std::is_same<io, double>::value), "the lean layout streams the fp64 workspace as it is");
    MS.ws = reinterpret_cast<const real*>(ws_lin) + (size_t)b * NS * LMPC_LIN_RECORD;
    MS.buf = reinterpret_cast<real*>(reinterpret_cast<unsigned char*>(TT) + (KS > 0 ? (LMPC_TERM_CELLS + 6 * LMPC_SS_STRIDE(P.S)) * sizeof(treal) : 0));
  }
  const treal tinf = treal(INFINITY);
  PT_DECL

  // ---------------- load: linearisation records, per-knot data, constant tables ----------------
  // (lmpc_solve_setup.hip.h: every load of the phase in one flight -- two at KQ = 7, more for the longer single-precision records)
  lmpc_load_problem<real, io, TEAM::THREADS, TEAM::CLASS, LEAN, TEAM::LEARN>(
      P, B, b, tid, L, ws_lin, x_ic, u_ic, T_ref, bl, br, vref, s_shift);
  tm.sync();
  PT_MARK(0)

  // ---------------- slot ownership ----------------
  // slot j = SLOT0 + lane + 64 q (SLOT0: the first slot of this wave)  ->  knot i = j / 11, kind sl = j % 11.  Kinds 0..9 constrain the primal
  // component (z[0..7], v[0..1]) at offset sl of the knot record; kind 10 is the track boundary
  // row pair on e_y (offset 1) which also carries the shared slack sigma.  Everything a slot needs
  // is reduced to LDS offsets and flag bits here so that the per-iteration row code is branch-free
  // (its loads batch and the slots of a lane interleave): an absent row keeps t = 1, lam = 0 and a
  // clear flag; a lane's surplus slots (j >= 11 N) point at a dead record inside the factor's work
  // matrices, so their loads and stores are harmless.
  const bool has_sigma = P.has_sigma != 0;
  const int KNB = NS * L.stride;                     // knot 0, offset from the LDS base (doubles)
  const int JB = KNB + N * LMPC_KNOT_STRIDE + TL_W;  // dead record (34 cells of W)
  const int CTB = KNB + N * LMPC_KNOT_STRIDE + TL_CT;
  int o_val[KQ];  // the constrained value; its Newton step sits at +10 (rhs0) and +20 (rhs1)
  int o_hl[KQ];   // the row pair's bounds (hi, lo): box table for kinds 0..9, knot record for the boundary
  int s_gf[KQ];   // gradient recipe: ct index of the coefficient on the value | on its partner << 8 | (partner offset + 1) << 16,
                  // and flags << 20: F_UP / F_LO row exists, F_SIG boundary slot carrying sigma, F_QLIN takes the linear
                  // vx cost, F_MOVE owns a moving primal component, F_EY boundary slot, F_SCH boundary slot of a knot >= 1
  real s_tu[KQ], s_tl[KQ], s_lu[KQ], s_ll[KQ], s_pu[KQ], s_pl[KQ];
  real m_rows = 0.0;
#pragma unroll
  for (int q = 0; q < KQ; ++q) {
    const int j = TEAM::SLOT0 + lane + 64 * q;
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
          const int k = uslot ? sl - SL_U : sl - SL_V;  // row of the 2x2 block (Qu on u, Sv on v)
          on = uslot ? i >= 1 : i <= N - 2;
          if (on) {
            ca = (uslot ? CT_QU : CT_SV) + 3 * k;        // diagonal entry
            cb = (uslot ? CT_QU : CT_SV) + 2 * k + 1 - k;  // [k][1-k]
          }
          pd = k == 0 ? 1 : -1;
        }
      } else {
        hi = lds[kb + KN_BHL];  // real(bl) - marg, real(br) + marg of the knot, as the load left them
        lo = lds[kb + KN_BHL + 1];
        on = has_sigma || i >= 1;
      }
    }
    const bool au = on && (hi < inf), al = on && (lo > -inf);
    const bool eys = valid && sl == SL_EY;
    const int fl = (au ? F_UP : 0) | (al ? F_LO : 0) | ((eys && has_sigma) ? F_SIG : 0) | ((valid && sl == 3) ? F_QLIN : 0) |
             ((valid && sl < SL_EY && (i >= 1 || sl >= SL_V)) ? F_MOVE : 0) | (eys ? F_EY : 0) | ((eys && i >= 1) ? F_SCH : 0);
    s_gf[q] = ca | (cb << 8) | ((pd + 1) << 16) | (fl << 20) | (sl << 27);  // (bits 27..30: the slot kind, for the polish's scaled step)
    m_rows += (au ? 1.0 : 0.0) + (al ? 1.0 : 0.0);
    s_tu[q] = s_tl[q] = 1.0;
    s_lu[q] = s_ll[q] = 0.0;
    s_pu[q] = s_pl[q] = 0.0;
  }
  // cell next to a boundary slot's weight that takes the sigma coupling coefficient (dead cell otherwise)
  // (a table integer read by itself goes through the team's table(): the empty asm below where the team's tables are opaque)
  auto flags = [&](int q) { return TEAM::table(s_gf[q]) >> 20; };
  // where the slot writes its barrier weight / gradient entry: the rhs0 cell of its component, or the boundary cell
  auto o_w = [&](int q) { return TEAM::table(o_val[q]) + ((flags(q) & F_EY) ? KN_EY - 1 : KN_R0); };
  auto o_csig = [&](int q) { return (flags(q) & F_EY) ? TEAM::table(o_val[q]) + (KN_CSIG - 1) : JB + KN_CSIG; };
  auto bounds = [&](int q) { return *reinterpret_cast<const real2*>(&lds[TEAM::table(o_hl[q])]); };
  // The slot's three table entries as the row phases of the iteration read them.  Where lmpc_opaque_slots says so they pass
  // through an empty asm first: every LDS address of a slot is loop-invariant, so the optimiser hoists all of them out of the
  // iteration -- eight addresses per slot where the tables hold three integers --, the allocator spills them, and each use then
  // waits on its own scratch reload (`scratch_load_dword; s_waitcnt vmcnt(0); ds_read`: a gradient evaluation at KQ = 11 was ~60 of
  // those in a row).  Behind the asm the addresses are recomputed from the tables with a handful of integer instructions.
  // (the two-wave kernels likewise: without it their gradient took 53 k cycles per iteration at N = 60 against 23 k in the one-wave kernel)
  struct SlotRef { int ov, oh, gf; };
  auto slot = [&](int q) {
    SlotRef r{o_val[q], o_hl[q], s_gf[q]};
    if constexpr (TEAM::OPAQUE_SLOTS) asm volatile("" : "+v"(r.ov), "+v"(r.oh), "+v"(r.gf));
    return r;
  };
  // (the short-horizon tracking kernels keep the hoisted addresses -- the opaque tables cost them 1-3 % -- except at the sites of
  //  lmpc_opaque_sites, where the address is a select on the slot's flags: bit 0 the coupling cell in the row phase, 1 the rhs1 cell
  //  the gradient clears, 2 the coupling cell in the Schur sums, 3 the primal update)
  auto slot_at = [&](int q, int site) {
    SlotRef r{o_val[q], o_hl[q], s_gf[q]};
    if constexpr (TEAM::OPAQUE_SLOTS) {
      asm volatile("" : "+v"(r.ov), "+v"(r.oh), "+v"(r.gf));
    } else if ((SITES >> site) & 1) {
      asm volatile("" : "+v"(r.gf));
    }
    return r;
  };
  auto r_flags = [](const SlotRef& r) { return r.gf >> 20; };
  auto r_w = [&](const SlotRef& r) { return r.ov + ((r_flags(r) & F_EY) ? KN_EY - 1 : KN_R0); };
  auto r_csig = [&](const SlotRef& r) { return (r_flags(r) & F_EY) ? r.ov + (KN_CSIG - 1) : JB + KN_CSIG; };
  auto r_bounds = [&](const SlotRef& r) { return *reinterpret_cast<const real2*>(&lds[r.oh]); };
  // ---------------- LMPC: simplex rows lambda_j >= 0, one safe-set point per lane and k < KS ----------------
  // (racing_mpc.cpp:484-504).  The points are centred on the first one (valid because 1'lambda = 1):
  // all sums below then run over O(1) offsets instead of absolute abscissae.
  const int S = P.S;
  SimplexRows<treal, KS> sx;
  treal lm_cold = 0.0;  // the cold start's simplex weight, 1 / (points kept)
  if constexpr (KS > 0) {
    treal* const UL = TT + TL_UL;
    sx.ul = UL;
    if (lane < 6) TT[TL_E + lane] = treal(P.chs2[lane]);
    // The safe set of this problem: as arrays (ss_x [6][S][B], ss_j [S][B]: lmpc_ss_query_batch wrote them), or BY REFERENCE
    // (P.ss_idx, round 5): S codes from lmpc_ss_query_idx_batch, each naming a row of the lap store and which of its three
    // unrolled copies; the point is read from the store (48 contiguous bytes, L2-resident: the whole store is < 0.2 MB) and its
    // cost-to-go recomputed from the row -- the same expressions as lmpc_ss_query_kernel uses, so both routes give the same bits.
    const bool by_ref = P.ss_idx != nullptr;
    auto ss_point = [&](int j, io (&pt)[6], io& jv) {  // point j of this problem's safe set (storage precision) and its J (not yet relative)
      const int code = P.ss_idx[(size_t)j * B + b];
      if (code < 0 || (code >> 2) >= P.ss_rows || (code & 3) == 3) {  // (no point; or not a code of this store: never read out of bounds)
#pragma unroll
        for (int k = 0; k < 6; ++k) pt[k] = io(0);
        jv = io(0);
        return;
      }
      const int row = code >> 2, rep = code & 3;
      int l = 0;
      for (int t = 1; t < P.ss_laps; ++t) l = (row >= P.ss_off[t]) ? t : l;
      const int n = P.ss_npts[l], jj = row - P.ss_off[l];
      const double* src = P.ss_store + (size_t)row * 6;
#pragma unroll
      for (int k = 0; k < 6; ++k) pt[k] = io(src[k] + (k == 0 ? (rep - 1) * P.ss_L : 0.0));
      jv = io((double)(n - 1 - jj) + (1 - rep) * (double)(n - 1));
    };
    io c0[6], j0v = io(0);  // the differences are formed in the storage precision, the abscissa relative to the shift
    if (by_ref) {
      ss_point(0, c0, j0v);
    } else {
#pragma unroll
      for (int k = 0; k < 6; ++k) c0[k] = ss_x[((size_t)k * S) * B + b];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) sx.ss0[k] = treal(k == 0 ? c0[k] - s_shift : c0[k]);
#pragma unroll
    for (int q = 0; q < KS; ++q) {
      const int j = lane + 64 * q;
      sx.on[q] = j < S;
      sx.uz[q] = 6 * (sx.on[q] ? j : S);
      if (by_ref) {
        io pt[6], jv = io(0);
        if (sx.on[q]) {
          ss_point(j, pt, jv);
#pragma unroll
          for (int k = 0; k < 6; ++k) UL[6 * j + k] = treal(pt[k] - c0[k]);
        }
        sx.j[q] = sx.on[q] ? treal(jv - j0v) : treal(0);
      } else {
#pragma unroll
        for (int k = 0; k < 6; ++k)
          if (sx.on[q]) UL[6 * j + k] = treal(ss_x[((size_t)k * S + j) * B + b] - c0[k]);
        sx.j[q] = sx.on[q] ? treal(ss_j[(size_t)j * B + b]) : treal(0);
      }
      if (q == 0 && lane < 6) UL[6 * S + lane] = treal(0);  // the zero point
    }
    wave_fence();
    // A point that repeats the one before it is dropped (round 5): it adds nothing to the hull, and two free copies of one point
    // make the explicit points' system C_A singular -- the interior point's steps and the polish's multiplier steps then carry
    // noise of 1e-4.  The padding of a set with fewer than S points is such a run (racing_mpc.cpp:263-272 repeats the last point
    // S - n_found times): with 64 points found and 96 copies the answers were 5e-3 from the dense optimum, status OPTIMAL
    // (scratch/r5/pad_check.py; the twin has the same rule).  X, U, dU are those of the full set; a run's weight sits on its first
    // point, the copies report lambda = 0.
    real n_on = 0.0;
#pragma unroll
    for (int q = 0; q < KS; ++q) {
      const int j = lane + 64 * q;
      bool dup = false;
      if (sx.on[q] && j > 0) {
        if (by_ref) {
          dup = P.ss_idx[(size_t)j * B + b] == P.ss_idx[(size_t)(j - 1) * B + b];
        } else {
          dup = ss_j[(size_t)j * B + b] == ss_j[(size_t)(j - 1) * B + b];
#pragma unroll
          for (int k = 0; k < 6; ++k) dup = dup && UL[6 * j + k] == UL[6 * (j - 1) + k];
        }
      }
      sx.on[q] = sx.on[q] && !dup;
      sx.uz[q] = 6 * (sx.on[q] ? j : S);
      sx.j[q] = sx.on[q] ? sx.j[q] : treal(0);
      n_on += sx.on[q] ? real(1) : real(0);
    }
    const treal inv_on = treal(1) / treal(uni(wave_sum<TEAM::RID>(n_on)));
    lm_cold = inv_on;
#pragma unroll
    for (int q = 0; q < KS; ++q) {
      sx.lm[q] = sx.on[q] ? inv_on : treal(0);
      sx.t[q] = sx.on[q] ? inv_on : treal(1);
      sx.l[q] = 0.0;
      sx.p[q] = 0.0;
      sx.dl[q] = 0.0;
      sx.aidx[q] = -1;
      m_rows += sx.on[q] ? 1.0 : 0.0;
    }
    treal umax = 0.0;  // largest u_j'E u_j of the (centred) points
#pragma unroll
    for (int q = 0; q < KS; ++q) {
      treal uq[6], v = 0.0;
      sx.load_u(q, lane, uq);
#pragma unroll
      for (int k = 0; k < 6; ++k) v += treal(P.chs2[k]) * uq[k] * uq[k];
      umax = fmax(umax, v);
    }
    sx.tau = uni(treal(TAU_REL) * wave_max<TEAM::RID>(umax));
    sx.m = 0;
  }
  const real m_tot = tm.sum(m_rows);
  const real inv_m = TEAM::uniform(real(1) / m_tot);

  // knot-0 feasibility: the state box applies to x_0 = x_ic (racing_mpc.cpp:147,201)
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
    feasible = tm.all(ok);
  }

  // The row sigma >= 0 (racing_mpc.cpp:536) is redundant and not carried: replacing a negative sigma by 0 loosens every
  // boundary row and lowers q_boundary sigma^2, so the QP without the row has the same optimum.  Carried, it is a
  // degenerate row whenever the boundary is inactive (sigma* = 0, multiplier 0) and costs two to three iterations.
  real sigma = 0.0;

  const real tau = 0.995, mu0 = 0.1, thr_frac = 0.5;
  int status = LMPC_SOLVE_MAX_ITER, it = 0;
  real mu = 0.0, rdmax = 0.0, rd_check = 0.0, last_step = 0.0, hsig = 0.0, ce = 0.0, mu_prev = inf;
  bool distress = false;
  const int max_iter = feasible ? P.max_iter : 0;
  typedef polish_limits<real> pol;
  const bool polish_on = P.polish >= 0;
  bool polished = false, pol_early_done = false, reentry = false, stall_moving = false;
  int pol_rounds = 0;
  // results: layout by strides (lmpc_set_output_layout): [component][knot][batch] by default -- what batch-parallel consumers
  // read coalesced -- or [batch][knot][component], one problem's plan contiguous (the reference's DM layout).  One code
  // path: element (k, i) of problem b at k sk + i si + b sb.
  auto put_primal = [&]() {
    const size_t xk = P.out_aos ? 1 : (size_t)N * B, xi = P.out_aos ? 6 : (size_t)B, xb = P.out_aos ? (size_t)6 * N : 1;
    const size_t uk = P.out_aos ? 1 : (size_t)NS * B, ui = P.out_aos ? 2 : (size_t)B, ub = P.out_aos ? (size_t)2 * NS : 1;
    for (int e = tid; e < 6 * N; e += TEAM::THREADS) {
      const int k = e / N, i = e - k * N;
      X_out[k * xk + i * xi + b * xb] = io(L.kn(i)[k]) + (k == 0 ? s_shift : io(0));
    }
    for (int e = tid; e < 2 * NS; e += TEAM::THREADS) {
      const int k = e / NS, i = e - k * NS;
      U_out[k * uk + i * ui + b * ub] = io(L.kn(i + 1)[6 + k]);
      dU_out[k * uk + i * ui + b * ub] = io(L.kn(i)[8 + k]);
    }
  };
  // The active-set polish is a call (lmpc_polish_call above): the interior point's row state goes in by value, an accepted
  // attempt returns the wave-wide scalars and the simplex weights of the polished point (the point itself is in LDS), a
  // refused one has put everything back.
  bool pol_noise = false;
  auto polish_attempt = [&](int max_rounds) -> bool {
    PolishArgs<real, KQ, KS> pa;
    pa.max_rounds = max_rounds;
    pa.keep = reinterpret_cast<io*>(P.save) + (size_t)b * (10 * N - 4);
    pa.ws = MS.ws;
    pa.N = N;
    pa.S = P.S;
    pa.has_sigma = P.has_sigma;
    pa.have0 = MS.have0;
    pa.have1 = MS.have1;
    pa.pol_rounds = pol_rounds;
    pa.qsig = qsig;
    pa.inv_m = inv_m;
    pa.sigma = sigma;
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
      pa.o_val[q] = o_val[q];
      pa.o_hl[q] = o_hl[q];
      pa.s_gf[q] = s_gf[q];
      pa.s_tu[q] = s_tu[q];
      pa.s_tl[q] = s_tl[q];
      pa.s_lu[q] = s_lu[q];
      pa.s_ll[q] = s_ll[q];
    }
    pa.sx = sx;
    PolishResult<real, KS> pr;
    // (the warm-start kernels at two waves per SIMD keep the polish inline: their accepted attempts ARE the polish, and behind a call the
    //  closed loop loses 3 .. 5 %: 6.65 -> 6.43 M car-steps/s at 4096 cars, 12.5 -> 11.9 M at 16384)
    if constexpr (TEAM::POLISH_CALL && !WARM_INLINE)
      pr = TEAM::template polish_call<real, io>(pa);
    else
      pr = lmpc_polish<real, KQ, KS, io, TEAM>(pa);
    tm.after_polish();
    pol_rounds = uni(pr.pol_rounds);
#ifdef LMPC_PHASE_TIMING
    if constexpr (KS == 0) {  // (the learning kernels use buckets 13 .. 15 for their terminal block)
      pf.acc[13] += pr.prof[0];
      pf.acc[14] += pr.prof[1];
      pf.acc[15] += pr.prof[2];
      pf.acc[18] += pr.prof[3];
      pf.acc[19] += 1;
    }
#endif
    // what the interior point recomputes before it reads it again (predictor products -- multiplied by zero in the next
    // predictor pass --, the explicit-point bookkeeping, the Schur scalars) does not live across the polish
#pragma unroll
    for (int q = 0; q < KQ; ++q) s_pu[q] = s_pl[q] = 0.0;
    hsig = 0.0;
    ce = 0.0;
    if constexpr (KS > 0) {
#pragma unroll
      for (int q = 0; q < KS; ++q) {
        sx.p[q] = 0.0;
        sx.dl[q] = 0.0;
        sx.aidx[q] = -1;
      }
      sx.m = 0;
      sx.r1 = 0.0;
    }
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
      if constexpr (KS > 0) {
#pragma unroll
        for (int q = 0; q < KS; ++q) sx.lm[q] = pr.lm[q];
      }
    }
    return accepted;
  };

  // ---------------- start point: minimiser of the cost over the dynamics alone ----------------
  // ... preceded, in a warm solve (lmpc_solve_batch_warm; fp64 tracking kernels), by an ACTIVE-SET attempt on the plan the caller
  // hands in -- the reference's X_optm_ref / U_optm_ref (racing_mpc.cpp:293-305), in the node the previous solution shifted by
  // one knot (racing_mpc_node.cpp:245-254).  Attempt 0: (1) the same zero-weight factorisation as the cold start; (2) the plan is
  // written into the rhs0 cells and rolled out under that factorisation's feedback, v = v^plan - K (z - z^plan): dynamically exact
  // about THIS linearisation, a few 1e-3 from the plan (which misses the new dynamics by the linearisation's change and x_0 by the
  // plant's step); (3) the working set is read off the PLAN: a polished optimum sits on its active bounds to rounding and the
  // boxes do not move with the shift (WARM_ACT); the boundary rows' bounds do, by the track's change over one knot (WARM_ACT_EY);
  // (4) the polish solves on that set, verifies the KKT conditions of this problem and repairs the set, WARM_ROUNDS times at
  // most.  Accepted: the optimum for about two iterations' worth of sweeps -- 92 .. 96 % of the periods of a closed loop at
  // N = 20 .. 60 on the serial twin (scratch/r5/warm_loop.py), iterations 6.5 -> 1.5 in the mean, answers those of the cold
  // solve to 1e-11.  Refused: attempt 1, the cold start, as if nothing had happened (the rounds spent are counted in `iters`).
  // The learning problem (round 6) takes the route with one more piece of the plan: the simplex weights of its terminal point --
  // the reference's convex_combi_optm_ref (set_initial(convex_combi_, ...), racing_mpc.cpp:281), P.warm_lam [S][B], aligned with
  // THIS call's safe-set points.  Their support is the working set of the simplex rows -- free where the plan's weight is positive,
  // held at zero elsewhere --, the weights themselves start the multiplier steps.  Without them there is nothing to start from
  // (all S weights free is more than the terminal block keeps explicit): the solve is cold.
  constexpr bool WARM_BUILT = WARMK && sizeof(real) == 8 && sizeof(io) == 8;
  const bool warm = WARM_BUILT && P.warm_X != nullptr && polish_on && feasible && (KS == 0 || P.warm_lam != nullptr);
  bool warm_done = false;
  for (int attempt = warm ? 0 : 1; attempt < 2 && !warm_done; ++attempt) {
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
      lds[o_w(q)] = 0.0;
      lds[o_csig(q)] = 0.0;
    }
    if constexpr (KS > 0) {  // lambda frozen at 1/S: terminal cost eps'D eps only
      if (lane < 36) TT[TL_PT + lane] = (lane % 7 == 0) ? TT[TL_E + lane / 7] : treal(0);
    }
    tm.sync();
    PT_MARK(1)
    if constexpr (TEAM::CHAIN) riccati_factor<FORM, (KS > 0), false>(L, MS, lane, TT + TL_PT);
    PT_MARK(16)
    if constexpr (WARM_BUILT) {
      if (attempt == 0) {
        // the plan in the solver's variables into the rhs0 cells: z_i = [x_i; u_{i-1}] (knot 0: the measured state and the applied
        // input), v_i = (u_i - u_{i-1}) / t_i
        const double* const WX = P.warm_X;
        const double* const WU = P.warm_U;
        for (int e = lane; e < 10 * N; e += 64) {
          const int i = e / 10, o = e - 10 * i;
          real val = 0.0;
          if (o < 6) {
            val = i == 0 ? KN0[o] : real(WX[((size_t)o * N + i) * B + b]);
          } else if (o < 8) {
            val = i == 0 ? KN0[o] : real(WU[((size_t)(o - 6) * NS + (i - 1)) * B + b]);
          } else if (i < NS) {
            const real up = i == 0 ? KN0[o - 2] : real(WU[((size_t)(o - 8) * NS + (i - 1)) * B + b]);
            val = (real(WU[((size_t)(o - 8) * NS + i) * B + b]) - up) / real(T_ref[(size_t)i * B + b]);
          }
          L.kn(i)[KN_R0 + o] = val;
        }
        wave_sync();
        feedback_rollout<FORM, true>(L, MS, lane);
        // the plan's boundary slack, then its working set (the interior point's row state is what the polish classifies by:
        // a held row gets lam = 1 > t = 0, every other row lam = 0 <= t = its slack)
        real vw[KQ];
        real2 hlw[KQ];
        real sgmax = 0.0;
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
          vw[q] = lds[o_val[q] + KN_R0];
          hlw[q] = bounds(q);
          const int f = flags(q);
          if (f & F_SIG) sgmax = fmax(sgmax, fmax((f & F_UP) ? vw[q] - hlw[q].x : real(0), (f & F_LO) ? hlw[q].y - vw[q] : real(0)));
        }
        sigma = uni(wave_max<TEAM::RID>(sgmax));
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
          const int f = flags(q);
          const real sg = (f & F_SIG) ? sigma : real(0), tolw = (f & F_EY) ? real(WARM_ACT_EY) : real(WARM_ACT);
          const real su = hlw[q].x + sg - vw[q], sd = vw[q] + sg - hlw[q].y;
          const bool hu = (f & F_UP) && su <= tolw, hd = (f & F_LO) && sd <= tolw;
          s_tu[q] = hu ? real(0) : fmax(su, real(0));
          s_tl[q] = hd ? real(0) : fmax(sd, real(0));
          s_lu[q] = hu ? real(1) : real(0);
          s_ll[q] = hd ? real(1) : real(0);
          s_tu[q] = (f & F_UP) ? s_tu[q] : real(1);
          s_tl[q] = (f & F_LO) ? s_tl[q] : real(1);
        }
        bool lam_ok = true;
        if constexpr (KS > 0) {  // the simplex rows' working set and start from the plan's weights (copies of a dropped run: ignored)
          treal lw[KS], lsum = 0.0;
#pragma unroll
          for (int q = 0; q < KS; ++q) {
            const int j = lane + 64 * q;
            lw[q] = sx.on[q] ? fmax(treal(P.warm_lam[(size_t)(j < S ? j : 0) * B + b]), treal(0)) : treal(0);
            lsum += lw[q];
          }
          lsum = uni(wave_sum<TEAM::RID>(lsum));
          lam_ok = lsum > treal(0);
          const treal inv = lam_ok ? treal(1) / lsum : treal(0);
#pragma unroll
          for (int q = 0; q < KS; ++q) {
            const treal lm = lw[q] * inv;
            const bool fr = sx.on[q] && lm > treal(WARM_ACT);
            sx.lm[q] = lm;
            sx.t[q] = sx.on[q] ? (fr ? lm : treal(0)) : treal(1);  // (the polish classifies by l > t: held)
            sx.l[q] = sx.on[q] ? (fr ? treal(0) : treal(1)) : treal(0);
            sx.p[q] = 0.0;
            sx.dl[q] = 0.0;
            sx.aidx[q] = -1;
          }
        }
        wave_sync();
        if (lam_ok && polish_attempt(P.warm_rounds > 0 ? P.warm_rounds : WARM_ROUNDS)) {
          polished = true;
          status = LMPC_SOLVE_OPTIMAL;
          warm_done = true;
        } else {  // refused: the cold start sets everything up again (row state: at the end of its Newton step)
          sigma = 0.0;
#pragma unroll
          for (int q = 0; q < KQ; ++q) {
            s_tu[q] = s_tl[q] = 1.0;
            s_lu[q] = s_ll[q] = 0.0;
          }
          if constexpr (KS > 0) {
#pragma unroll
            for (int q = 0; q < KS; ++q) {
              sx.lm[q] = sx.on[q] ? lm_cold : treal(0);
              sx.t[q] = sx.on[q] ? lm_cold : treal(1);
              sx.l[q] = 0.0;
              sx.p[q] = 0.0;
              sx.dl[q] = 0.0;
              sx.aidx[q] = -1;
            }
            sx.m = 0;
          }
        }
        continue;
      }
    }
    if constexpr (TEAM::CHAIN) feedback_rollout<FORM>(L, MS, lane);
    tm.after_chain();
    PT_MARK(17)
  }
  if constexpr (KS > 0) {
    treal ul[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < KS; ++q) {
      treal uq[6];
      sx.load_u(q, lane, uq);
#pragma unroll
      for (int k = 0; k < 6; ++k) ul[k] += uq[k] * sx.lm[q];
    }
    wave_sum_split<6, TEAM::RID>(ul, lane);
    if (lane < 6) {
      treal e = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k)
        if (k == lane) e = (treal(L.kn(N - 1)[k]) - sx.ss0[k]) - ul[k];
      TT[TL_EPS + lane] = e;
      TT[TL_TG + lane] = TT[TL_E + lane] * e;
    }
    wave_sync();
  }
  PT_MARK(1)

  // it == -1 is the start-point Newton step (all row weights zero, full step); it >= 0 the
  // interior-point iterations.  The iterations are the INNER loop; a polish attempt (a call) sits between two runs of it
  // (outer loop: at most twice round).
  it = -1;
  for (; !warm_done;) {
  int hand_over = 0;  // why the interior point stopped: 0 for good (status says why), 1 the early polish attempt, 2 the one at its exit,
                      // 3 out of iterations but close (single precision): a last attempt
  for (; it <= max_iter; ++it) {
    const bool ipm = it >= 0;
    // ======== gradient: cost gradient + row coefficients, written by the component owner (into the rhs0 cells) ========
    // (a function of the iterate and of (sigma_c mu, pm) only: with the fused factorisation the predictor's is assembled BEFORE the
    //  factorisation, which consumes it; the rhs1 cells then hold the barrier weights and are not cleared here)
    treal eeps[6] = {0, 0, 0, 0, 0, 0};  // E eps of this iterate (safe-set block), in scalar registers
    auto load_eeps = [&]() {
      if constexpr (KS > 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) eeps[k] = uni(TT[TL_E + k] * TT[TL_EPS + k]);
      }
    };
    real sgsum0 = 0.0;
    auto gradient = [&](const int pass, const real smu, const real pm) -> real {
      const bool fused = FUSEK && fuse && ipm;
      real sgsum = 0.0;
      if constexpr (KS > 0) {
        if (ipm) {
          PT_MARK(12)
          // right-hand side r_j = -bl_j (dx = 0): sums over the eliminated points, the explicit ones through LDS
          treal bs[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
          for (int q = 0; q < KS; ++q) {
            treal itf, uq[6];
            sx.load_u(q, lane, uq);
            const treal rj = sx.on[q] ? -simplex_bl(sx.lm[q], sx.t[q], sx.l[q], sx.p[q], sx.j[q], uq, treal(smu), treal(pm), eeps, itf) : treal(0);
            if (sx.aidx[q] >= 0) TT[TL_RA + sx.aidx[q]] = rj;
            const treal w = (sx.on[q] && sx.aidx[q] < 0) ? rj * itf : treal(0);
            bs[6] += w;
#pragma unroll
            for (int k = 0; k < 6; ++k) bs[k] += uq[k] * w;
          }
          wave_sum_split<7, TEAM::RID>(bs, lane);
          wave_fence();
          PT_MARK(13)
          treal beta[6], h[6], nu;
#pragma unroll
          for (int k = 0; k < 6; ++k) beta[k] = bs[k];
          term_solve_u(TT, lane, sx.m, beta, bs[6], sx.r1, h, nu);
          PT_MARK(14)
          if (lane < 6) {  // terminal gradient onto x_T: E eps + pT, pT = -h
            treal hs = h[0];
#pragma unroll
            for (int k = 1; k < 6; ++k) hs = (lane == k) ? h[k] : hs;
            TT[TL_TG + lane] = TT[TL_E + lane] * TT[TL_EPS + lane] - hs;
          }
          wave_fence();
          PT_MARK(15)
        }
      }
#pragma unroll
      for (int q0 = 0; q0 < KQ; q0 += QC) {
        real val[QC], par[QC], ca[QC], cb[QC], ql[QC];
        real2 hl[QC];
        SlotRef sr[QC];
#pragma unroll
        for (int qq = 0; qq < QC; ++qq) {
          const int q = q0 + qq;
          if (q >= KQ) continue;
          sr[qq] = slot(q);
          const int gr = sr[qq].gf, ov = sr[qq].ov;
          val[qq] = lds[ov];
          hl[qq] = r_bounds(sr[qq]);
          par[qq] = lds[ov + ((gr >> 16) & 3) - 1];
          ca[qq] = lds[CTB + (gr & 0xff)];
          cb[qq] = lds[CTB + ((gr >> 8) & 0xff)];
          ql[qq] = lds[ov + (KN_QLIN - 3)];
        }
#pragma unroll
        for (int qq = 0; qq < QC; ++qq) {
          const int q = q0 + qq;
          if (q >= KQ) continue;
          // (two waves read the slot's tables afresh for the arithmetic, as their text did: the copies of the load loop, kept alive
          //  across it, cost w2<11> / w2<14> 12 / 20 spilled VGPRs -- profiles/iteration_one_body.md)
          if constexpr (TEAM::OPAQUE) sr[qq] = slot(q);
          const int f = r_flags(sr[qq]);
          const real sg = (f & F_SIG) ? sigma : 0.0;
          const real itu = frcp(s_tu[q]), itl = frcp(s_tl[q]);
          real cu = s_lu[q] * itu * (val[qq] - sg + s_tu[q] - hl[qq].x) + (smu - pm * s_pu[q]) * itu;
          real cd = s_ll[q] * itl * (-val[qq] - sg + s_tl[q] + hl[qq].y) + (smu - pm * s_pl[q]) * itl;
          cu = (ipm && (f & F_UP)) ? cu : 0.0;
          cd = (ipm && (f & F_LO)) ? cd : 0.0;
          const real g = ca[qq] * val[qq] + cb[qq] * par[qq] + ((f & F_QLIN) ? ql[qq] : real(0));  // (zero coefficients on a boundary slot)
          lds[r_w(sr[qq])] = g + cu - cd;
          if (pass == 0 && !fused) {
            const SlotRef sz = ((SITES & 2) && !TEAM::OPAQUE_SLOTS) ? slot_at(q, 1) : sr[qq];
            lds[(r_flags(sz) & F_EY) ? JB + KN_EY : r_w(sz) + 10] = 0.0;
          }
          sgsum += (f & F_SIG) ? (cu + cd) : real(0);
        }
        if constexpr (QC < KQ) ISSUE_ORDER();
      }
      tm.sync();
      PT_MARK(12)
      for (int i = tid; i < N; i += TEAM::THREADS) {
        real* kn = L.kn(i);
        kn[KN_R0 + 1] += kn[KN_EY];
        if (pass == 0 && !fused) kn[KN_R1 + 1] = (i >= 1) ? kn[KN_CSIG] : 0.0;
      }
      if constexpr (KS > 0) {  // terminal gradient of the safe-set block onto x_T (lanes 0..5 != EY lanes' cells)
        wave_sync();
        if (lane < 6) L.kn(N - 1)[KN_R0 + lane] += real(TT[TL_TG + lane]);
      }
      tm.sync();
      return sgsum;
    };
    // ======== rows: complementarity, residual, barrier weights ========
    if (ipm) {
      real musum = 0.0, rdl = 0.0, eysum = 0.0;
#pragma unroll
      for (int q0 = 0; q0 < KQ; q0 += QC) {  // (QC slots at a time: the whole row in one go where the registers allow it)
        real val[QC];
        real2 hl[QC];
        SlotRef sr[QC];
#pragma unroll
        for (int qq = 0; qq < QC; ++qq) {
          const int q = q0 + qq;
          if (q >= KQ) continue;
          sr[qq] = slot(q);
          val[qq] = lds[sr[qq].ov];
          hl[qq] = r_bounds(sr[qq]);
        }
#pragma unroll
        for (int qq = 0; qq < QC; ++qq) {
          const int q = q0 + qq;
          if (q >= KQ) continue;
          if constexpr (TEAM::OPAQUE) sr[qq] = slot(q);
          const int f = r_flags(sr[qq]);
          const real sg = (f & F_SIG) ? sigma : 0.0;
          const real thu = s_lu[q] * frcp(s_tu[q]), thd = s_ll[q] * frcp(s_tl[q]);
          musum += s_lu[q] * s_tu[q] + s_ll[q] * s_tl[q];
          rdl = fmax(rdl, (f & F_UP) ? fabs(val[qq] - sg + s_tu[q] - hl[qq].x) : real(0));
          rdl = fmax(rdl, (f & F_LO) ? fabs(-val[qq] - sg + s_tl[q] + hl[qq].y) : real(0));
          lds[r_w(sr[qq]) + (fuse ? ((f & F_EY) ? KN_TEY - KN_EY : KN_R1 - KN_R0) : 0)] = thu + thd;
          // (NOT a simplification to make: where this address is formed decides the bits.  With the address taken from sr[] the
          //  difference below sits in the block of its two products and is fused with one of them, v_fma_f64 thd, -thu unrounded;
          //  o_csig(q) has an empty asm in one arm of its conditional, which keeps control flow between them, and the two-wave kernels
          //  have always computed the rounded difference -- profiles/iteration_one_body.md, section 2)
          if constexpr (TEAM::ROUNDED_CSIG)
            lds[o_csig(q)] = (f & F_SIG) ? (thd - thu) : 0.0;
          else
            lds[r_csig(((SITES & 1) && !TEAM::OPAQUE_SLOTS) ? slot_at(q, 0) : sr[qq])] = (f & F_SIG) ? (thd - thu) : 0.0;
          eysum += (f & F_SIG) ? (thu + thd) : real(0);
        }
        if constexpr (QC < KQ) ISSUE_ORDER();
      }
      if constexpr (KS > 0) {
        PT_MARK(2)
        // ---- which points stay explicit this iteration: the (at most MA_MAX) smallest theta below tau ----
        treal thq[KS];
#pragma unroll
        for (int q = 0; q < KS; ++q) {
          thq[q] = sx.on[q] ? sx.l[q] * frcp(sx.t[q]) : tinf;
          sx.aidx[q] = -1;
        }
        if (lane < 6 * MA_MAX) TT[TL_UA + lane] = 0.0;            // unused slots: u = 0, theta = 1, rhs = 0
        if (lane < MA_MAX) {
          TT[TL_THA + lane] = 1.0;
          TT[TL_RA + lane] = 0.0;
        }
        wave_fence();
        int m = 0;
        for (int a = 0; a < MA_MAX; ++a) {
          treal cand = tinf;
          int cq = 0;
#pragma unroll
          for (int q = 0; q < KS; ++q) {
            const bool better = sx.aidx[q] < 0 && thq[q] < sx.tau && thq[q] < cand;
            cand = better ? thq[q] : cand;
            cq = better ? q : cq;
          }
          const treal best = wave_min<TEAM::RID>(cand);
          if (!(best < tinf)) break;
          const int owner = __ffsll((long long)__ballot(cand == best)) - 1;  // the lowest lane holding the minimum
          if (lane == owner) {
#pragma unroll
            for (int q = 0; q < KS; ++q)
              if (q == cq) {
                sx.aidx[q] = a;
                treal uq[6];
                sx.load_u(q, lane, uq);
#pragma unroll
                for (int k = 0; k < 6; ++k) TT[TL_UA + a * 6 + k] = uq[k];
                TT[TL_THA + a] = thq[q];
              }
          }
          wave_fence();
          m = a + 1;
        }
        sx.m = m;
        wave_fence();
        // ---- sums over the eliminated points: T_B (21), a_B (6), s_B; and over all points: U lambda (6), sum lambda ----
        treal tt[21], av[14];
#pragma unroll
        for (int k = 0; k < 21; ++k) tt[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 14; ++k) av[k] = 0.0;
#pragma unroll
        for (int q = 0; q < KS; ++q) {
          const treal on = sx.on[q] ? 1.0 : 0.0;
          const treal itf = (sx.on[q] && sx.aidx[q] < 0) ? frcp(thq[q]) : treal(0);
          musum += real(on * sx.l[q] * sx.t[q]);
          rdl = fmax(rdl, real(on * fabs(-sx.lm[q] + sx.t[q])));
          int n = 0;
          treal uq[6];
          sx.load_u(q, lane, uq);
#pragma unroll
          for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int c = r; c < 6; ++c) tt[n++] += uq[r] * uq[c] * itf;
            av[r] += uq[r] * itf;
            av[7 + r] += uq[r] * sx.lm[q];
          }
          av[6] += itf;
          av[13] += sx.lm[q];
        }
        {  // 35 sums: 32 through the splitting butterfly, the last three on their own
          treal red[32], red3[3] = {av[11], av[12], av[13]};
#pragma unroll
          for (int k = 0; k < 21; ++k) red[k] = tt[k];
#pragma unroll
          for (int k = 0; k < 11; ++k) red[21 + k] = av[k];
          wave_sum_split<32, TEAM::RID>(red, lane);
          wave_sum_split<3, TEAM::RID>(red3, lane);
#pragma unroll
          for (int k = 0; k < 21; ++k) tt[k] = red[k];
#pragma unroll
          for (int k = 0; k < 11; ++k) av[k] = red[21 + k];
          av[11] = red3[0];
          av[12] = red3[1];
          av[13] = red3[2];
        }
        sx.r1 = 1.0 - av[13];
        {
          treal F[36], aB[6];
          int n = 0;
#pragma unroll
          for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int c = r; c < 6; ++c) {
              F[r * 6 + c] = tt[n];
              F[c * 6 + r] = tt[n];
              ++n;
            }
            aB[r] = av[r];
          }
#pragma unroll
          for (int k = 0; k < 6; ++k) F[k * 6 + k] += 1.0 / fmax(TT[TL_E + k], treal(1e-30));  // (a zero weight: that component of eps is free)
          term_factor_u(TT, lane, F, aB, av[6], m);
        }
        if (lane < 6) {
          treal e = 0.0;
#pragma unroll
          for (int k = 0; k < 6; ++k)
            if (k == lane) e = (treal(L.kn(N - 1)[k]) - sx.ss0[k]) - av[7 + k];
          TT[TL_EPS + lane] = e;
        }
        wave_fence();
      }
      {
        real red[2] = {musum, eysum};
        tm.sum2(red);
        musum = red[0];
        hsig = qsig + red[1];
      }
      rdmax = tm.max(rdl);  // (two waves: the two barriers above also publish the barrier weights for the factorisation)
      hsig = TEAM::uniform(hsig);
      mu = TEAM::uniform(musum * inv_m);
      // (see the step-length rule; far from feasibility mu may rise legitimately: IAC at 60 m/s into a corner)
      // (reentry: the same iterate a second time -- after a refused polish, or on the way to the final one: none of the
      // bookkeeping repeats)
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
      // primal infeasibility: on a feasible problem the row residual contracts by (1 - alpha) per iteration; not
      // losing a tenth over five iterations while still large (step lengths stuck below ~2 %) ends the solve (this
      // also bounds the straggler that would otherwise hold its CU slot for max_iter iterations).  "Not halved" is
      // too tight: feasible problems with a slow start (IAC at 60 m/s into a corner) contract by 0.6-0.8 per five.
      if (!again_here && it % 5 == 0) {
        if (it >= 10 && rdmax > lim::rd_infeasible && rdmax > real(0.9) * rd_check) {
          status = LMPC_SOLVE_INFEASIBLE;
          break;
        }
        rd_check = rdmax;
      }
      if (it == max_iter) {
        // single precision, out of iterations with the rows (nearly) feasible: the complementarity of an fp32 recursion can
        // hover just above its floor for good (seen on one IAC problem of 8192 that the fp64 kernel solves in 9 iterations).
        // The polish does not care how the interior point stopped -- it verifies what it returns -- so it gets the iterate;
        // refused, the status stays MAX_ITER (and the two-pass entries hand the problem to the fp64 kernel).
        if (sizeof(real) == 4 && polish_on && max_iter > 0 && mu <= real(1e-3) && rdmax <= real(10) * lim::rd_ok) hand_over = 3;
        break;
      }
      // the early attempt: the active set is usually settled two iterations before the interior point's own tolerance
      if constexpr (pol::early) {
        if (polish_on && !pol_early_done && mu <= real(pol::mu_early) && rdmax <= real(pol::rd_early)) {
          pol_early_done = true;
          hand_over = 1;
          break;
        }
      }
      tm.published();
      PT_MARK(2)
      if constexpr (FUSEK) {
        if (fuse) {
          load_eeps();
          sgsum0 = gradient(0, real(0), real(0));
          PT_MARK(4)
        }
      }
      if constexpr (TEAM::CHAIN) {
        if (sizeof(real) == 8 && mu <= real(JOSEPH_MU)) {  // (single precision stops at mu ~ 2e-6)
          if (FUSEK && fuse)
            riccati_factor<FORM, (KS > 0), (sizeof(real) == 8), FUSEK>(L, MS, lane, TT + TL_PT, KN_R1, KN_TEY);
          else
            riccati_factor<FORM, (KS > 0), (sizeof(real) == 8)>(L, MS, lane, TT + TL_PT);
        } else {
          if (FUSEK && fuse)
            riccati_factor<FORM, (KS > 0), false, FUSEK>(L, MS, lane, TT + TL_PT, KN_R1, KN_TEY);
          else
            riccati_factor<FORM, (KS > 0), false>(L, MS, lane, TT + TL_PT);
        }
      }
      tm.after_chain();
      PT_MARK(3)
    }

    real sigc = 0.0, alpha = 1.0, dsigma = 0.0;
    bool numerics_failed = false, stalled = false;
    if (!(FUSEK && fuse && ipm)) load_eeps();
    real d_val[KQ];
    const int npass = ipm ? 2 : 1;
    for (int pass = 0; pass < npass; ++pass) {
      const real smu = (pass == 1) ? sigc * mu : 0.0, pm = (pass == 1) ? 1.0 : 0.0;
      real sgsum = sgsum0;  // sum of boundary-row coefficients entering the sigma gradient
      if (!(FUSEK && fuse && ipm && pass == 0)) {
        sgsum = gradient(pass, smu, pm);
        PT_MARK(4)
      }
      // ======== Newton step: predictor together with the Schur vector, then the corrector ========
      if constexpr (TEAM::CHAIN) {
        if (pass == 0 && ipm && has_sigma) {
          if (FUSEK && fuse)
            riccati_solve<FORM, 2, FUSEK>(L, MS, lane, pf);
          else
            riccati_solve<FORM, 2>(L, MS, lane, pf);
        } else
          riccati_solve<FORM, 1>(L, MS, lane, pf);
      }
      tm.after_chain();
      PT_MARK(5)
      // ======== step of every constrained value; boundary slack by Schur complement ========
      // (QC == KQ: the steps and values are loaded once, here, and stay in registers across the reduction; otherwise chunk-wise,
      //  once for the Schur sums and again for the row steps)
      real dz0[QC == KQ ? KQ : 1], dz1[QC == KQ ? KQ : 1], val[QC == KQ ? KQ : 1];
      real2 hl[QC == KQ ? KQ : 1];
      if constexpr (QC == KQ) {
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
          dz0[q] = lds[TEAM::table(o_val[q]) + 10];
          dz1[q] = lds[TEAM::table(o_val[q]) + 20];
          val[q] = lds[TEAM::table(o_val[q])];
          hl[q] = bounds(q);
        }
      }
      if (!ipm) {
#pragma unroll
        for (int q = 0; q < KQ; ++q) d_val[q] = QC == KQ ? dz0[QC == KQ ? q : 0] : lds[slot(q).ov + 10];
        break;
      }
      if (has_sigma) {
        real red[3] = {0.0, 0.0, sgsum};  // c'dz (this rhs), c'e (Schur vector), sum of boundary coefficients
        if constexpr (QC == KQ) {
          real cs[KQ];
#pragma unroll
          for (int q = 0; q < KQ; ++q) cs[q] = lds[r_csig(slot_at(q, 2))];
#pragma unroll
          for (int q = 0; q < KQ; ++q) {
            const bool sch = (flags(q) & F_SCH) != 0;
            red[0] += sch ? cs[q] * dz0[q] : real(0);
            red[1] += sch ? cs[q] * dz1[q] : real(0);
          }
        } else {
#pragma unroll
          for (int q0 = 0; q0 < KQ; q0 += QC) {
            real cs[QC], e0[QC], e1[QC];
            SlotRef sr[QC];
#pragma unroll
            for (int qq = 0; qq < QC; ++qq) {
              const int q = q0 + qq;
              if (q >= KQ) continue;
              sr[qq] = slot(q);
              cs[qq] = lds[r_csig(sr[qq])];
              e0[qq] = lds[sr[qq].ov + 10];
              e1[qq] = lds[sr[qq].ov + 20];
            }
#pragma unroll
            for (int qq = 0; qq < QC; ++qq) {
              const int q = q0 + qq;
              if (q >= KQ) continue;
              const bool sch = (r_flags(sr[qq]) & F_SCH) != 0;
              red[0] += sch ? cs[qq] * e0[qq] : real(0);
              red[1] += sch ? cs[qq] * e1[qq] : real(0);
            }
            ISSUE_ORDER();
          }
        }
        tm.sum3(red);
        if (pass == 0) ce = red[1];
        const real qsg = qsig * sigma - red[2];
        dsigma = uni(-(qsg + red[0]) / (hsig + ce));
      }
      if constexpr (KS > 0) {
        // r_j = u_j'E dx_T - bl_j;  d lambda_j = (r_j - nu - u_j'h)/theta_j for the eliminated points, the explicit
        // ones from the small dense solve
        const real* knT = L.kn(N - 1);
        treal e[6], gs[7] = {0, 0, 0, 0, 0, 0, 0}, rj[KS], itfq[KS];
#pragma unroll
        for (int k = 0; k < 6; ++k) e[k] = TT[TL_E + k] * treal(knT[KN_R0 + k] + dsigma * knT[KN_R1 + k]);
#pragma unroll
        for (int q = 0; q < KS; ++q) {
          treal itf, uq[6];
          sx.load_u(q, lane, uq);
          treal r = -simplex_bl(sx.lm[q], sx.t[q], sx.l[q], sx.p[q], sx.j[q], uq, treal(smu), treal(pm), eeps, itf);
#pragma unroll
          for (int k = 0; k < 6; ++k) r += uq[k] * e[k];
          r = sx.on[q] ? r : 0.0;
          rj[q] = r;
          itfq[q] = itf;
          if (sx.aidx[q] >= 0) TT[TL_RA + sx.aidx[q]] = r;
          const treal w = (sx.on[q] && sx.aidx[q] < 0) ? r * itf : treal(0);
          gs[6] += w;
#pragma unroll
          for (int k = 0; k < 6; ++k) gs[k] += uq[k] * w;
        }
        wave_sum_split<7, TEAM::RID>(gs, lane);
        wave_fence();
        treal beta[6], h[6], nu;
#pragma unroll
        for (int k = 0; k < 6; ++k) beta[k] = gs[k];
        term_solve_u(TT, lane, sx.m, beta, gs[6], sx.r1, h, nu);
#pragma unroll
        for (int q = 0; q < KS; ++q) {
          treal uh = 0.0, uq[6];
          sx.load_u(q, lane, uq);
#pragma unroll
          for (int k = 0; k < 6; ++k) uh += uq[k] * h[k];
          const treal dB = (rj[q] - nu - uh) * itfq[q];
          const treal dA = TT[TL_XA + (sx.aidx[q] >= 0 ? sx.aidx[q] : 0)];
          sx.dl[q] = sx.on[q] ? (sx.aidx[q] >= 0 ? dA : dB) : treal(0);
        }
      }
      // ======== row steps; largest feasible step as 1 / max(1, max -dt/t, max -dlam/lam) ========
      auto row_step = [&](bool on, treal t, treal lam, treal pprod, treal rd, treal cdy, treal& dt_, treal& dl_,
                          treal& it_) {  // (the simplex rows: always fp64)
        it_ = frcp(t);
        dt_ = on ? (-rd - cdy) : 0.0;
        dl_ = on ? (-lam + (treal(smu) - treal(pm) * pprod) * it_ - lam * it_ * dt_) : 0.0;
      };
      real dtu[KQ], dlu[KQ], dtl[KQ], dll[KQ];
      real rmax = 1.0;
      bool finite_step = true;
#pragma unroll
      for (int q0 = 0; q0 < KQ; q0 += QC) {
        real e0[QC], e1[QC], ev[QC];
        real2 eh[QC];
        SlotRef sr[QC];
#pragma unroll
        for (int qq = 0; qq < QC; ++qq) {
          const int q = q0 + qq;
          if (q >= KQ) continue;
          sr[qq] = slot(q);
          if constexpr (QC == KQ) {
            e0[qq] = dz0[q], e1[qq] = dz1[q], ev[qq] = val[q], eh[qq] = hl[q];
          } else {
            e0[qq] = lds[sr[qq].ov + 10];
            e1[qq] = lds[sr[qq].ov + 20];
            ev[qq] = lds[sr[qq].ov];
            eh[qq] = r_bounds(sr[qq]);
          }
        }
#pragma unroll
        for (int qq = 0; qq < QC; ++qq) {
          const int q = q0 + qq;
          if (q >= KQ) continue;
          if constexpr (TEAM::OPAQUE) sr[qq] = slot(q);
          const int f = r_flags(sr[qq]);
          const real dval = e0[qq] + dsigma * e1[qq];
          d_val[q] = dval;
          finite_step = finite_step && (fabs(dval) < inf);
          const real sg = (f & F_SIG) ? sigma : 0.0, dsg = (f & F_SIG) ? dsigma : 0.0;
          const real itu = frcp(s_tu[q]), itl = frcp(s_tl[q]);
          const real a = (f & F_UP) ? -(ev[qq] - sg + s_tu[q] - eh[qq].x) - (dval - dsg) : 0.0;
          const real bq = (f & F_UP) ? -s_lu[q] + (smu - pm * s_pu[q]) * itu - s_lu[q] * itu * a : 0.0;
          const real c = (f & F_LO) ? -(-ev[qq] - sg + s_tl[q] + eh[qq].y) - (-dval - dsg) : 0.0;
          const real d = (f & F_LO) ? -s_ll[q] + (smu - pm * s_pl[q]) * itl - s_ll[q] * itl * c : 0.0;
          dtu[q] = a;
          dlu[q] = bq;
          dtl[q] = c;
          dll[q] = d;
          rmax = fmax(rmax, fmax(-a * itu, -bq * frcp(fmax(s_lu[q], lim::tiny))));
          rmax = fmax(rmax, fmax(-c * itl, -d * frcp(fmax(s_ll[q], lim::tiny))));
        }
        if constexpr (QC < KQ) ISSUE_ORDER();
      }
      if constexpr (KS > 0) {
#pragma unroll
        for (int q = 0; q < KS; ++q) {
          treal dt_, dl_, it_;
          row_step(sx.on[q], sx.t[q], sx.l[q], sx.p[q], -sx.lm[q] + sx.t[q], -sx.dl[q], dt_, dl_, it_);
          rmax = fmax(rmax, real(fmax(-dt_ * it_, -dl_ * frcp(fmax(sx.l[q], treal(1e-300))))));
        }
      }
      rmax = tm.max(finite_step ? rmax : inf);
      if (!(rmax < inf) || !(dsigma == dsigma)) {
        // a Newton step that is not a number (the Schur complement of sigma or the 2x2 H cancelled completely -- in
        // practice single precision on its last iteration): keep the iterate, report it by what it has reached
        numerics_failed = true;
        break;
      }
      const real amax = TEAM::uniform(real(1) / rmax);
      if (pass == 1) {
        alpha = TEAM::uniform(fmin(real(1), tau * amax));
        if (TEAM::NBHD && distress) {  // (fp64 arithmetic, N <= 40 -- KQ <= 7 of the class: see below)
          // A problem whose complementarity has gone UP once gets the wide-neighbourhood rule from then on: the step is
          // cut back until no complementarity product falls below NBHD_GAMMA times their mean.  Mehrotra's iteration can
          // otherwise leave the neighbourhood of the central path and cycle -- seen on a learning problem whose safe set
          // offers two nearly exchangeable points: products at 0.01 and 300 times mu, mu bouncing between 6e-6 and 2e-5
          // up to the iteration cap while the dense solver finds the optimum (19 iterations with the rule).  Problems
          // whose mu falls monotonically (all but a few per thousand) never enter this branch.  The single-precision
          // instantiations do without it: their mu is noisy at its floor, and the branch costs the mixed learning kernel
          // 280 B of scratch per lane at two waves per SIMD (3.13 -> 2.89 M solves/s).  Nor do the N > 40 instantiations,
          // which already spill their row state: the branch costs them another 260 B per lane (N = 60: +9 % time).
          for (int trial = 0; trial < NBHD_TRIALS; ++trial) {
            real sl = 0.0, pmin = inf;
#pragma unroll
            for (int q = 0; q < KQ; ++q) {
              const int f = flags(q);
              const real pu = (s_tu[q] + alpha * dtu[q]) * (s_lu[q] + alpha * dlu[q]);
              const real pl = (s_tl[q] + alpha * dtl[q]) * (s_ll[q] + alpha * dll[q]);
              sl += pu + pl;  // (an absent row has lam = 0, d lam = 0: no contribution)
              pmin = fmin(pmin, fmin((f & F_UP) ? pu : inf, (f & F_LO) ? pl : inf));
            }
            if constexpr (KS > 0) {
#pragma unroll
              for (int q = 0; q < KS; ++q) {
                treal dt_, dl_, it_;
                row_step(sx.on[q], sx.t[q], sx.l[q], sx.p[q], -sx.lm[q] + sx.t[q], -sx.dl[q], dt_, dl_, it_);
                const real pr = real((sx.t[q] + treal(alpha) * dt_) * (sx.l[q] + treal(alpha) * dl_));
                sl += sx.on[q] ? pr : real(0);
                pmin = fmin(pmin, sx.on[q] ? pr : inf);
              }
            }
            pmin = tm.min(pmin);  // (a statement of its own: two waves pair their exchanges by order, which C++ leaves open inside an expression)
            if (pmin >= real(NBHD_GAMMA) * tm.sum(sl) * inv_m) break;
            alpha = TEAM::uniform(alpha * real(0.6));
          }
        }
      }
      real sacc = 0.0;
#pragma unroll
      for (int q = 0; q < KQ; ++q) {
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
      if constexpr (KS > 0) {
#pragma unroll
        for (int q = 0; q < KS; ++q) {
          treal dt_, dl_, it_;
          row_step(sx.on[q], sx.t[q], sx.l[q], sx.p[q], -sx.lm[q] + sx.t[q], -sx.dl[q], dt_, dl_, it_);
          if (pass == 0) {
            sacc += sx.on[q] ? real((sx.t[q] + treal(amax) * dt_) * (sx.l[q] + treal(amax) * dl_)) : real(0);
            sx.p[q] = dt_ * dl_;
          } else {
            sx.t[q] += treal(alpha) * dt_;
            sx.l[q] += treal(alpha) * dl_;
            sx.lm[q] += treal(alpha) * sx.dl[q];
            sacc += sx.on[q] ? real(sx.t[q] * sx.l[q]) : real(0);
          }
        }
      }
      sacc = tm.exchanged(sacc);  // (two waves: ONE exchange ahead of both arms; one wave reduces where it reads, in the arm)
      if (pass == 1) {
        // no further progress: rows feasible, complementarity already small, and the corrector step would not lower it
        // (the Newton direction has reached the accuracy of the factorisation): keep the current primal iterate
        sacc = tm.sum_of(sacc);
        if (rdmax <= lim::rd_ok && mu <= real(STALL_MU) && sacc * inv_m >= mu) stalled = true;
      }
      if (pass == 0) {
        sacc = tm.sum_of(sacc);
        const real ratio = (sacc * inv_m) / mu;
        sigc = TEAM::uniform(ratio * ratio * ratio);
        tm.published();
      }
    }

    if (numerics_failed) {
      status = (mu <= real(10) * tol && rdmax <= lim::rd_ok) ? LMPC_SOLVE_OPTIMAL : LMPC_SOLVE_MAX_ITER;
      // (what the interior point has reached is polished like a converged iterate; single precision short of its tolerance
      // but close gets the last attempt of the out-of-iterations exit above: refused, it stays MAX_ITER)
      hand_over = (status == LMPC_SOLVE_OPTIMAL && polish_on) ? 2 : 0;
      if (sizeof(real) == 4 && status != LMPC_SOLVE_OPTIMAL && polish_on && mu <= real(1e-3) && rdmax <= real(10) * lim::rd_ok) hand_over = 3;
      break;
    }
    if (stalled) {
      // (round 6: a stall is not convergence when the Newton step it declines would still move the iterate -- the point is kept and handed to the
      //  polish as before, but unless the polish verifies it the status is MAX_ITER: oracle/c/lmpc_oracle.c, STALL_STEP, has the problem)
      real cand = 0.0;  // the step the stall declines to take, in the reference's scaled units (like the polish's steps)
#pragma unroll
      for (int q = 0; q < KQ; ++q) cand = fmax(cand, (flags(q) & F_MOVE) ? fabs(alpha * d_val[q]) * real(slot_inv_scale((TEAM::table(s_gf[q]) >> 27) & 15)) : real(0));
      stall_moving = sizeof(real) == 8 && tm.max(cand) > real(STALL_STEP);
      status = (stall_moving && !polish_on) ? LMPC_SOLVE_MAX_ITER : LMPC_SOLVE_OPTIMAL;
      hand_over = polish_on ? 2 : 0;
      break;
    }
    // ======== primal update by the component owners ========
    PT_MARK(6)
    real stepmax = 0.0;
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
      const SlotRef sr = slot_at(q, 3);
      const bool mv = (r_flags(sr) & F_MOVE) != 0;
      const real dz = mv ? alpha * d_val[q] : 0.0;
      lds[mv ? sr.ov : JB + q] += dz;
      stepmax = fmax(stepmax, fabs(dz));
    }
    tm.publish(ipm);
    if (ipm) {
      last_step = tm.max(stepmax);
      if (has_sigma) sigma = TEAM::uniform(sigma + alpha * dsigma);
    } else {
      // ---- slacks and multipliers at the start point: t = max(slack, 0.5 range), lam = mu0 / t ----
      real val[KQ];
      real2 hl[KQ];
      int fl[KQ];
#pragma unroll
      for (int q = 0; q < KQ; ++q) {
        const SlotRef sr = slot(q);
        val[q] = lds[sr.ov];
        hl[q] = r_bounds(sr);
        fl[q] = r_flags(sr);
      }
#pragma unroll
      for (int q = 0; q < KQ; ++q) {
        real range = ((fl[q] & (F_UP | F_LO)) == (F_UP | F_LO)) ? (hl[q].x - hl[q].y) : 1.0;
        if (!(range > real(1e-3))) range = real(1e-3);
        const real thr = thr_frac * range;
        if (fl[q] & F_UP) {
          s_tu[q] = fmax(hl[q].x - val[q], thr);
          s_lu[q] = mu0 / s_tu[q];
        }
        if (fl[q] & F_LO) {
          s_tl[q] = fmax(val[q] - hl[q].y, thr);
          s_ll[q] = mu0 / s_tl[q];
        }
      }
      sigma = 0.0;
      if constexpr (KS > 0) {
#pragma unroll
        for (int q = 0; q < KS; ++q) sx.l[q] = sx.on[q] ? treal(mu0) / sx.t[q] : treal(0);
      }
    }
  }
  if (hand_over == 0) break;
  tm.sync();
  if (polish_attempt(pol::rounds | (hand_over >= 2 ? POLISH_EXIT : 0))) {
    polished = true;
    status = LMPC_SOLVE_OPTIMAL;
    break;
  }
  if (hand_over == 3) break;  // refused after the last iteration: out of iterations it is
  if (hand_over == 2 || !pol::early) {  // refused at the exit: the interior point's own answer stands
    status = LMPC_SOLVE_OPTIMAL;
    // ... unless the refusal itself says that answer cannot be trusted to the contract (fp64, round 5).  A held set that is
    // CONSISTENT -- no negative multiplier, no violated row -- whose multiplier steps nevertheless do not settle (last step
    // above step_tol, or a held row not met to `feas`, after four steps) is a problem whose linear algebra is noisier than
    // 1e-6: seen at vx < 0.6 m/s with N >= 36, where the RK4 step map's spectral radius is ~25 per stage (DESIGN.md section
    // 3, "where it has to converge") and the steps bounce at 1e-4.  The interior point's iterate, computed with the same
    // sweeps, was then 1e-6 .. 2e-3 from the dense optimum with status OPTIMAL (tests/dispatch_sweep.py, one problem of
    // 1024 at eighteen horizons).  It now says LMPC_SOLVE_MAX_ITER: stopped short of the stated accuracy.  No problem of
    // the bench distributions takes this branch (twin, 4096 / 1024 problems per family).
    // (round 6: likewise a STALLED iterate whose declined step would still have moved it by more than STALL_STEP)
    if (sizeof(real) == 8 && (pol_noise || stall_moving)) status = LMPC_SOLVE_MAX_ITER;
    break;
  }
  reentry = true;  // refused early: the interior point goes on from the same iterate (same `it`; the rows phase puts its
                   // barrier weights back into the records)
  }
  PT_MARK(7)
  if (it < 0) it = 0;
  it += pol_rounds;  // (a polish round costs about what an iteration does and is counted as one)
  if (!feasible) status = LMPC_SOLVE_INFEASIBLE;
  if constexpr (KS > 0) {
    // hard hull equality (the penalty limit, LMPC_HARD_HULL_WEIGHT): a terminal state the hull cannot reach leaves a
    // residual the weight does not close -- the reference's QP is infeasible there
    if (P.hard_hull && status == LMPC_SOLVE_OPTIMAL) {
      wave_sync();
      treal worst = 0;
#pragma unroll
      for (int k = 0; k < 6; ++k) worst = fmax(worst, fabs(TT[TL_EPS + k]) * treal(slot_inv_scale(k)));
      if (worst > treal(LMPC_HARD_HULL_RESIDUAL)) status = LMPC_SOLVE_INFEASIBLE;
    }
  }
  // two-pass mixed precision: an answer the fp32 iteration could not verify -- or did not reach: out of iterations, or
  // "infeasible" by single-precision residuals -- is marked for the fp64 kernel behind it, which has the last word
  if (P.flag_unverified && (status != LMPC_SOLVE_OPTIMAL || (polish_on && !polished))) status = LMPC_SOLVE_UNVERIFIED;

  // ---------------- write back: X [6][N][B], U, dU [2][N-1][B] ----------------
  tm.sync();
  put_primal();
  if constexpr (KS > 0) {
    if (lam_out) {
#pragma unroll
      for (int q = 0; q < KS; ++q)
        if (lane + 64 * q < S) lam_out[(size_t)(lane + 64 * q) * B + b] = sx.on[q] ? io(sx.lm[q]) : io(0);  // (a dropped copy: 0)
    }
  }
  if (TEAM::CHAIN && lane == 0) {  // (two waves: the chain wave reports, and the clocks of the profiling build are its own)
    status_out[b] = status;
    iters_out[b] = it;
    if constexpr (WARMK) {
      if (P.warm_flag) P.warm_flag[b] = warm_done ? 1 : 0;  // (explicit: until round 6 callers inferred it from iters <= 4)
    }
#ifdef LMPC_PHASE_TIMING
    if (kkt_out) {
      if constexpr (LEAN) pf.acc[5] = MS.waited;  // (cycles inside ModelStream::wait of the interior point's own sweeps -- also counted in their phases)
      for (int k = 0; k < 16; ++k) kkt_out[k * (size_t)B + b] = (io)pf.acc[k];
      kkt_out[16 * (size_t)B + b] = (io)pf.w0;               // 100 MHz wall clock at start
      kkt_out[17 * (size_t)B + b] = (io)wall_clock64();      // ... at end
      unsigned hwid, xcc;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      kkt_out[18 * (size_t)B + b] = (io)hwid;
      kkt_out[19 * (size_t)B + b] = (io)(xcc & 0xf);
      for (int k = 16; k < 20; ++k) kkt_out[(k + 4) * (size_t)B + b] = (io)pf.acc[k];
    }
#else
    if (kkt_out) {
      kkt_out[0 * (size_t)B + b] = io(last_step);
      kkt_out[1 * (size_t)B + b] = io(rdmax);
      kkt_out[2 * (size_t)B + b] = io(mu);
      kkt_out[3 * (size_t)B + b] = io(sigma);
    }
#endif
  }
}

template <typename real, int KQ, int KS, typename io>
__global__ __launch_bounds__(64, lmpc_waves_per_simd(sizeof(real), KQ, KS)) void lmpc_solve_kernel(
    lmpc_params P, int B, const io* __restrict__ ws_lin, const io* __restrict__ x_ic,
    const io* __restrict__ u_ic, const io* __restrict__ T_ref, const io* __restrict__ bl,
    const io* __restrict__ br, const io* __restrict__ vref, const io* __restrict__ ss_x,
    const io* __restrict__ ss_j, io* __restrict__ lam_out, io* __restrict__ X_out,
    io* __restrict__ U_out, io* __restrict__ dU_out, int* __restrict__ status_out,
    int* __restrict__ iters_out, io* __restrict__ kkt_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];  // one symbol for every instantiation
  // XCD-aware problem assignment: consecutive workgroups go round-robin to the 8 XCDs (each with its own L2), while
  // consecutive problems share 64-byte lines in the [field][knot][batch] arrays.  Workgroup w takes problem
  // (w mod 8) * ceil(B / 8) + w / 8, so each XCD owns a contiguous eighth of the batch and the 8-byte strided
  // accesses of neighbouring problems merge in that XCD's L2 instead of reaching HBM as partial lines.
  // With a launch order (longest job first from the previous solve's iteration counts, lmpc_set_launch_order) workgroup
  // w takes problem launch_order[w]: the hardware starts workgroups in index order, so the long problems go first and the
  // short ones fill the tail of the second residency round.
  int b = (int)(blockIdx.x & 7) * ((B + 7) >> 3) + (int)(blockIdx.x >> 3);
  if (P.launch_order) {
    const int n = P.order_count ? *P.order_count : B;  // (a list: the workgroups past its end have nothing to do)
    b = (int)blockIdx.x < n ? P.launch_order[blockIdx.x] : B;
  }
  if (b >= B) return;
  lmpc_solve_problem<real, KQ, KS, io>(P, B, b, lds_raw, ws_lin, x_ic, u_ic, T_ref, bl, br, vref, ss_x, ss_j, lam_out, X_out, U_out,
                                       dU_out, status_out, iters_out, kkt_out);
}

// Second pass of a mixed-precision solve (lmpc_solve_batch_mixed): the problems the fp32 iteration marked
// LMPC_SOLVE_UNVERIFIED, solved in fp64.  `list` [count] holds them (lmpc_collect_unverified_kernel); a small fixed grid
// of workgroups takes list entries in turn -- launching one workgroup per problem of the batch to have 99 % of them
// return at once costs more than the solves (38 KB of LDS and 500 registers to allocate per workgroup: 1.3 ms per 8192).
// The solve is a CALL here, not inlined into the loop: with the 3000-line body inlined under a loop the <double, 7, 3>
// instance computed garbage (nondeterministically; the same body without the loop, or called once per workgroup, is bit
// for bit the direct kernel -- scratch/r3_cleanup_dbg.py); behind a call boundary every instance is.  Round 4 met the same
// family deterministically in <double, 7, 0> and bisected it ("the register-starved instantiations":
// the answers of these 460-to-512-register functions depend on how the compiler parks spilled scalars in VGPR lanes; wait
// counts, post-RA scheduling and the machine verifier are ruled out): the noinline works around exactly that -- a call
// boundary is the one thing that has kept every build of this family right.  The callee names the workgroup's dynamic
// LDS block itself, so its accesses stay in the LDS address space.
template <typename real, int KQ, int KS, typename io>
__device__ __attribute__((noinline)) void lmpc_solve_problem_call(
    const lmpc_params& P, const int B, const int b, const io* __restrict__ ws_lin, const io* __restrict__ x_ic,
    const io* __restrict__ u_ic, const io* __restrict__ T_ref, const io* __restrict__ bl, const io* __restrict__ br,
    const io* __restrict__ vref, const io* __restrict__ ss_x, const io* __restrict__ ss_j, io* __restrict__ lam_out,
    io* __restrict__ X_out, io* __restrict__ U_out, io* __restrict__ dU_out, int* __restrict__ status_out,
    int* __restrict__ iters_out, io* __restrict__ kkt_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  lmpc_solve_problem<real, KQ, KS, io, true>(P, B, b, lds_raw, ws_lin, x_ic, u_ic, T_ref, bl, br, vref, ss_x, ss_j, lam_out, X_out, U_out,
                                             dU_out, status_out, iters_out, kkt_out);
}

template <typename real, int KQ, int KS, typename io>
__global__ __launch_bounds__(64, lmpc_waves_per_simd(sizeof(real), KQ, KS)) void lmpc_cleanup_kernel(
    lmpc_params P, int B, const int* __restrict__ list, const int* __restrict__ count, const io* __restrict__ ws_lin,
    const io* __restrict__ x_ic, const io* __restrict__ u_ic, const io* __restrict__ T_ref, const io* __restrict__ bl,
    const io* __restrict__ br, const io* __restrict__ vref, const io* __restrict__ ss_x,
    const io* __restrict__ ss_j, io* __restrict__ lam_out, io* __restrict__ X_out,
    io* __restrict__ U_out, io* __restrict__ dU_out, int* __restrict__ status_out,
    int* __restrict__ iters_out, io* __restrict__ kkt_out) {
  const int n = __builtin_amdgcn_readfirstlane(*count);
  for (int w = blockIdx.x; w < n; w += gridDim.x) {
    const int b = __builtin_amdgcn_readfirstlane(list[w]);  // (wave-uniform: keep the problem index in a scalar register)
    lmpc_solve_problem_call<real, KQ, KS, io>(P, B, b, ws_lin, x_ic, u_ic, T_ref, bl, br, vref, ss_x, ss_j, lam_out, X_out, U_out, dU_out,
                                              status_out, iters_out, kkt_out);
    wave_fence();
  }
}

// The warm-start solve (lmpc_solve_batch_warm) is a kernel of its own: compiled into lmpc_solve_kernel, the attempt's code changed
// the register allocation of the cold path -- 992 -> 1296 B of scratch per lane at KQ = 11, 1796 -> 2128 B at KQ = 14, 132 more
// spilled scalars in the headline kernel -- for callers that never pass a plan.  Same body, WARMK = true.
template <int KQ, int KS>
__global__ __launch_bounds__(64, lmpc_waves_per_simd(8, KQ, KS)) void lmpc_solve_warm_kernel(
    lmpc_params P, int B, const double* __restrict__ ws_lin, const double* __restrict__ x_ic, const double* __restrict__ u_ic,
    const double* __restrict__ T_ref, const double* __restrict__ bl, const double* __restrict__ br, const double* __restrict__ vref,
    const double* __restrict__ ss_x, const double* __restrict__ ss_j, double* __restrict__ lam_out,
    double* __restrict__ X_out, double* __restrict__ U_out, double* __restrict__ dU_out, int* __restrict__ status_out,
    int* __restrict__ iters_out, double* __restrict__ kkt_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  int b = (int)(blockIdx.x & 7) * ((B + 7) >> 3) + (int)(blockIdx.x >> 3);  // (as lmpc_solve_kernel)
  if (P.launch_order) {
    const int n = P.order_count ? *P.order_count : B;
    b = (int)blockIdx.x < n ? P.launch_order[blockIdx.x] : B;
  }
  if (b >= B) return;
  lmpc_solve_problem<double, KQ, KS, double, false, true>(P, B, b, lds_raw, ws_lin, x_ic, u_ic, T_ref, bl, br, vref, ss_x, ss_j, lam_out, X_out,
                                                          U_out, dU_out, status_out, iters_out, kkt_out);
}

#include "lmpc_solve_w2.hip.h"  // two wavefronts per problem: the fp64 tracking kernels for N >= 24 (round 6)
#define LMPC_W2_SIGNATURE(KQ)                                                                                            \
  __global__ void lmpc_solve_kernel_w2<KQ>(lmpc_params, int, const double*, const double*, const double*, const double*, \
                                           const double*, const double*, const double*, double*, double*, double*, int*, int*, double*);

#define LMPC_SOLVE_SIGNATURE(REAL, KQ, KS, IO)                                                                           \
  __global__ void lmpc_solve_kernel<REAL, KQ, KS, IO>(lmpc_params, int, const IO*, const IO*, const IO*, const IO*, const IO*, \
                                                       const IO*, const IO*, const IO*, const IO*, IO*, IO*, IO*, IO*, int*, int*, IO*);
#define LMPC_INSTANTIATE(REAL, KQ, KS, IO) template LMPC_SOLVE_SIGNATURE(REAL, KQ, KS, IO)
#define LMPC_INSTANTIATED_ELSEWHERE(REAL, KQ, KS, IO) extern template LMPC_SOLVE_SIGNATURE(REAL, KQ, KS, IO)
#ifdef LMPC_SINGLE_INSTANCE  // (ISA inspection: hipcc -S -DLMPC_SINGLE_INSTANCE="double, 4, 3, double")
#define LMPC_INSTANTIATE_X(...) LMPC_INSTANTIATE(__VA_ARGS__)
LMPC_INSTANTIATE_X(LMPC_SINGLE_INSTANCE)
#elif defined(LMPC_MINREG_TU)  // lmpc_lib_minreg.hip: the two kernels that translation unit exists for
LMPC_INSTANTIATE(float, 4, 2, double)
LMPC_INSTANTIATE(float, 4, 3, double)
#elif defined(LMPC_W2_TU)  // lmpc_lib_w2.hip: the two-wave kernels (a translation unit of their own: they rebuild in a minute)
template LMPC_W2_SIGNATURE(7)
template LMPC_W2_SIGNATURE(11)
template LMPC_W2_SIGNATURE(14)
#else
extern template LMPC_W2_SIGNATURE(7)
extern template LMPC_W2_SIGNATURE(11)
extern template LMPC_W2_SIGNATURE(14)
#define LMPC_INSTANTIATE_WARM(KQ, KS)                                                                                    \
  template __global__ void lmpc_solve_warm_kernel<KQ, KS>(lmpc_params, int, const double*, const double*, const double*, const double*,   \
                                                          const double*, const double*, const double*, const double*, const double*, double*, \
                                                          double*, double*, double*, int*, int*, double*);
LMPC_INSTANTIATE_WARM(2, 0)
LMPC_INSTANTIATE_WARM(4, 0)
LMPC_INSTANTIATE_WARM(7, 0)
LMPC_INSTANTIATE_WARM(11, 0)
LMPC_INSTANTIATE_WARM(14, 0)
// the learning problem's warm start (round 6): the horizons the reference ships for it (barc_lmpc N = 40, iac_car_lmpc N = 60) and
// BASELINE's N = 20, with 96 (KS = 2) and 160 (KS = 3) points
LMPC_INSTANTIATE_WARM(4, 2)
LMPC_INSTANTIATE_WARM(4, 3)
LMPC_INSTANTIATE_WARM(7, 2)
LMPC_INSTANTIATE_WARM(7, 3)
LMPC_INSTANTIATE_WARM(11, 2)
LMPC_INSTANTIATE_WARM(11, 3)
LMPC_INSTANTIATE(double, 2, 0, double)
LMPC_INSTANTIATE(double, 4, 0, double)
LMPC_INSTANTIATE(double, 7, 0, double)
LMPC_INSTANTIATE(double, 11, 0, double)
LMPC_INSTANTIATE(double, 14, 0, double)
LMPC_INSTANTIATE(double, 4, 2, double)
LMPC_INSTANTIATE(double, 4, 3, double)
LMPC_INSTANTIATE(double, 7, 2, double)
LMPC_INSTANTIATE(double, 7, 3, double)
LMPC_INSTANTIATE(double, 11, 2, double)  // iac_car_lmpc.param.yaml ships N = 60
LMPC_INSTANTIATE(double, 11, 3, double)
LMPC_INSTANTIATE(double, 14, 2, double)
LMPC_INSTANTIATE(double, 14, 3, double)
LMPC_INSTANTIATE(float, 4, 0, float)
LMPC_INSTANTIATE(float, 7, 0, float)
LMPC_INSTANTIATE(float, 11, 0, float)
LMPC_INSTANTIATE(float, 14, 0, float)
// mixed: fp32 interior-point iteration between fp64 arrays (io = double); the third kernel type, `treal` -- the simplex rows
// and the terminal elimination of the learning problem -- is double in every instantiation: F = D^-1 + U Theta^-1 U' has a
// condition number ~1e8 late in the iteration, which fp32 cannot carry
LMPC_INSTANTIATE(float, 4, 0, double)
LMPC_INSTANTIATE(float, 7, 0, double)
LMPC_INSTANTIATE(float, 11, 0, double)  // iac_car_tracking_mpc.param.yaml ships N = 80
LMPC_INSTANTIATE(float, 14, 0, double)
// the learning problem, N <= 23 (BASELINE configs[4]): instantiated in a translation unit of their own (lmpc_lib_minreg.hip),
// which is compiled with -mllvm -amdgpu-sched-strategy=iterative-minreg -- the most spill-bound kernel of the library is the one
// place where the minimum-register scheduler pays (131 against 184 spilled VGPRs, 9.93 against 10.65 ms per 32768, same bits;
// every other kernel is 3-20 % slower with it: profiles/r04_sched_strategies.md).  Here: declarations only.
LMPC_INSTANTIATED_ELSEWHERE(float, 4, 2, double)
LMPC_INSTANTIATED_ELSEWHERE(float, 4, 3, double)
// the fp64 second pass behind each of the mixed kernels above
#define LMPC_INSTANTIATE_CLEANUP(KQ, KS)                                                                                  \
  template __global__ void lmpc_cleanup_kernel<double, KQ, KS, double>(lmpc_params, int, const int*, const int*,          \
      const double*, const double*, const double*, const double*, const double*, const double*, const double*,           \
      const double*, const double*, double*, double*, double*, double*, int*, int*, double*);
LMPC_INSTANTIATE_CLEANUP(4, 0)
LMPC_INSTANTIATE_CLEANUP(7, 0)
LMPC_INSTANTIATE_CLEANUP(11, 0)
LMPC_INSTANTIATE_CLEANUP(14, 0)
LMPC_INSTANTIATE_CLEANUP(4, 2)
LMPC_INSTANTIATE_CLEANUP(4, 3)
// (the learning problem at N = 40 in mixed precision was built and measured: 1.16 M solves/s against 0.70 M in fp64, but
//  median 1.2e-3 / 99th percentile 1.5e-2 from the fp64 answers -- outside the 1e-3 the mixed entry states; not shipped)
#endif
