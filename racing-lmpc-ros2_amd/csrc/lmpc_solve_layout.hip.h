// lmpc_solve_layout.hip.h -- what a solve kernel's LDS block looks like and which form of the code each instantiation takes.
// Holds: the LDS record layout of both layouts (stage / knot / tail offsets, the lean records, slot kinds and flags, MROWS), the handles
// onto it (Lds, SimplexRows), the per-instantiation constexpr policy functions (waves per SIMD, lean layout, polish call, row chunks,
// opaque slot tables, fused backward sweep, chain addresses, the reductions' identity), each with the measurement that decided it, and the description of the
// three forms of a stage chain (ChainForm, StageCells, CHAIN_GET / CHAIN_PUT) that the one body per chain in lmpc_solve_kernel.hip is
// written against.  Needs: lmpc_device.h (record strides) and lmpc_wave.hip.h (LDS addresses, fences).
// Included by lmpc_solve_kernel.hip, i.e. by all three translation units (lmpc_lib.hip, lmpc_lib_minreg.hip, lmpc_lib_w2.hip).
#ifndef LMPC_SOLVE_LAYOUT_HIP_H_
#define LMPC_SOLVE_LAYOUT_HIP_H_

#include "lmpc_device.h"
#include "lmpc_wave.hip.h"

#define NSLOT 11
// resident waves per SIMD the register allocation is sized for: the fp64 tracking kernels up to N = 23 and every fp32
// kernel up to N = 40 run two (three for fp32, N <= 23); the fp64 LMPC and long-horizon kernels need the full file.
// (Three for the single-precision N <= 23 kernel, whose 10 KB records allow 16 per CU -- measured: 1.04 / 0.93 / 0.97 ms per
// 8192-batch at 2 / 3 / 4; the issue ceiling (LDS pipe, VALU) is ~12 % away.)
constexpr int lmpc_waves_per_simd(int real_bytes, int kq, int ks) {
  return real_bytes == 4 ? ((kq <= 4 && ks == 0) ? 3 : (kq <= 7 ? 2 : 1)) : ((ks == 0 && kq <= 4) ? 2 : 1);
}

#define SL_U 6
#define SL_V 8
#define SL_EY 10

// ---- LDS layout (doubles) ---------------------------------------------------------------------
// stage record i (stride 78): M[8][8]: column c of the stage model with the feedback gain appended,
//                               M[c][k] = [A B][k][c] (k < 6), M[c][6 + j] = K_j[c].  Row c starts at
//                               ST_ROW(c) = 8 c + 2 (c >> 1): the two-cell skew after every second row puts
//                               the eight rows on eight different 4-bank groups, so the per-lane row reads
//                               (b128, lane = row) are conflict-free; column reads (lane = column) stay
//                               contiguous.  The six skew cells and the tail of the record hold
//                               Hinv (h00,h01) @16 | (h11, dt) @34 | kff rhs0 [2] @52 | kff rhs1 [2] @70 | g[6] @72
// knot record i (stride 36):  z[8] v[2] @0 | rhs0: Th / q / d [10] @10 | rhs1: q / e [10] @20
//                             | csig @30 | eyT / eyD @31 | boundary row bounds (hi, lo) @32 | qlin_vx @34
// tail: P[8][10] @0 | W[8][10] @80 | Y[8][10] @160 | pvec[2 buf][2 rhs][8] @240 | consts @272 (48)
#define ST_ROW(c) (8 * (c) + 2 * ((c) >> 1))
#define ST_HI 16     // h00, h01
#define ST_HI11 34   // h11
#define ST_DT 35
#define ST_KFF(s) ((s) ? 70 : 52)
#define ST_G 72
#define KN_R0 10
#define KN_R1 20
#define KN_CSIG 30
#define KN_EY 31
#define KN_BHL 32
#define KN_QLIN 34
#define TL_P 0
#define TL_W 80
#define TL_Y 160
#define TL_PV 240
#define TL_CT 272
#define CT_QD 0
#define CT_QT 6
#define CT_QU 12
#define CT_SV 16
#define CT_HL 20    // box bounds of the ten primal components, (hi, lo) interleaved
#define CT_ZERO 40  // a 0.0 entry: coefficient slot for "no term"
#define CT_E 41     // 2 * convex_hull_slack (LMPC)

#define F_UP 1
#define F_LO 2
#define F_SIG 4
#define F_QLIN 8
#define F_MOVE 16
#define F_EY 32
#define F_SCH 64
// Row r of the 8x8 work matrices P, W, Y starts at MROWS(r) = 8 r + 2 (r >> 1) -- the stage records' skew (ST_ROW): the eight rows
// sit on eight different 4-bank groups (conflict-free b128 row reads, as with the stride of 10 doubles used until round 5), AND the
// rows of a 16-lane store group (r = 2g, 2g + 1) are 16 banks apart, so the element stores of W, Y, P -- ds_write_b64: contiguous
// 16-lane groups, 32 banks -- are conflict-free too; with the stride of 10 rows 2g and 2g + 1 overlapped in four banks: every one of
// the four stores per factor stage took 8 LDS cycles instead of 4 (40 % of the headline kernel's SQ_LDS_BANK_CONFLICT, round 6).
#define MROWS(r) (8 * (r) + 2 * ((r) >> 1))

template <typename real> struct vec2;
template <> struct vec2<double> { typedef double2 type; };
template <> struct vec2<float> { typedef float2 type; };

// Register-resident state of the LMPC simplex rows lambda_j >= 0 (KS safe-set points per lane); empty for
// the tracking kernel so that it costs it nothing.
template <typename real, int KS>
struct SimplexRows {
  bool on[KS];
  int aidx[KS];  // slot of the point among the explicit ones of this iteration, -1: eliminated through 1/theta
  real lm[KS], t[KS], l[KS], p[KS], j[KS], dl[KS];
  real sv[KS];  // lambda at the start of a polish (restored when it is refused)
  const real* ul;  // the (centred) points in LDS, point-major: component k of point j at ul[6 j + k], S points -- read-only
                   // after the load, 36 registers (KS = 3) the iteration's row state needs more.  A point is 48 bytes = three
                   // 16-byte reads; 16 consecutive lanes at a 48-byte stride cover all 64 banks once, so the reads are
                   // conflict-free.  A lane slot past S reads the zero point stored behind the last one (uz[q] = its index).
  int uz[KS];      // 6 * (index of the point this lane's slot q reads)
  __device__ __forceinline__ void load_u(int q, int lane, real (&u)[6]) const {
    const real* p = ul + uz[q];
#pragma unroll
    for (int k = 0; k < 6; ++k) u[k] = p[k];
  }
  real ss0[6];
  real r1;   // 1 - 1'lambda
  real tau;  // theta below which a point is kept explicit
  int m;     // explicit points of this iteration
};
template <typename real>
struct SimplexRows<real, 0> {};

template <typename real>
struct Lds {
  real* base;
  int N;
  int stride;  // of a stage record: LMPC_STAGE_STRIDE, or LMPC_LEAN_STAGE_STRIDE in the lean layout (below)
  bool chain_prio;  // CHAIN_PRIO around the serial stage chains (a compile-time constant where the sweeps are inlined)
  __device__ __forceinline__ real* st(int i) const { return base + i * stride; }
  __device__ __forceinline__ real* kn(int i) const { return base + (N - 1) * stride + i * LMPC_KNOT_STRIDE; }
  __device__ __forceinline__ real* tail() const { return base + (N - 1) * stride + N * LMPC_KNOT_STRIDE; }
};

// ---- the LEAN layout (fp64, N > 40) -----------------------------------------------------------------------------------
// At long horizons the stage records are what limits residency: 78 doubles per stage, 48 of them the stage model [A B],
// which the iteration only reads.  The lean layout keeps the model OUT of the records: every sweep streams it from the
// linearisation workspace (L2 / MALL resident, written by lmpc_linearize_kernel just before) through two chunk buffers of
// LN_CHUNK stages each, filled by asynchronous global -> LDS copies (global_load_lds_dwordx4: no registers, no ds_write)
// one chunk ahead of the sweep (ModelStream, lmpc_solve_kernel.hip).  A stage record shrinks to what the factorisation produces:
//     K_j[c] @ 2 c + j (c < 8) | Hinv (h00, h01) @16, h11 @18 | dt @19 | kff rhs0 [2] @20 | kff rhs1 [2] @22        (24)
// and a chunk slot holds the workspace record as it is: ABt[8][6] (row c of it = column c of [A B]: the rows the backward
// sweeps read are contiguous 48-byte runs on distinct banks, the columns the forward sweep reads are stride-6) | g [6].
// N = 60: 57 KB -> 38 KB per problem, 2 -> 4 resident problems per CU (the register file allows no more); N = 80: 2 -> 3.
#define LN_CHUNK LMPC_LEAN_CHUNK  // (lmpc_device.h: the host sizes the two chunk buffers with the same constants)
#define LN_REC LMPC_LIN_RECORD
#define LN_HI 16
#define LN_HI11 18
#define LN_DT 19
#define LN_KFF(s) ((s) ? 22 : 20)
// Which kernels take it: the fp64 kernels from LMPC_LEAN_MIN_KQ = 11 slots per lane on (lmpc_device.h; the host's lmpc_is_lean is
// the same test)
constexpr bool lmpc_lean(int real_bytes, int kq) { return real_bytes == 8 && kq >= LMPC_LEAN_MIN_KQ; }

// Where the polish is a call: every fp64 kernel calls it (lmpc_polish_call), the fp32 kernels inline it.  The sweeps take a fresh
// lane value (FRESH_LANE, lmpc_wave.hip.h) in every instantiation.  Measured per instantiation in round 4
// (profiles/r04_polish_forms.md: {inline, call} x {fresh, not}, every (KQ, KS), checksums against the round-3 build):
//   * fp64, one wave per SIMD (KQ >= 7 or the learning problem: the instantiations that live in VGPRs + AGPRs): a CALL.  The call
//     form computes bit for bit what the round-3 kernel computed, at every horizon and for both problems; the inlined function
//     does not: with FRESH_LANE in the factorisation AND the vector solve the <double, 7, 0> instance (N = 24 .. 40) returns
//     different -- wrong -- answers (72 of 8192 IAC problems "infeasible"), the same wrong answers whatever the post-RA schedule
//     or the wait counts, and the right ones again with SGPR spills sent to memory instead of VGPR lanes, or at -O2 (DESIGN.md
//     section 4, "the register-starved instantiations").  The call costs the callee's prologue / epilogue and the spills around
//     the call site, ~1 KB of scratch traffic per lane and call, and buys -5 .. -16 % of the kernel time from N = 60 on and for
//     the learning problem from N = 40 on (nothing either way at N = 40 tracking).
//   * fp64, two waves per SIMD (tracking up to N = 23: the headline): a CALL too, since round 6.  Round 4 measured the two forms at the
//     same time (0.872 inlined against 0.868 ms per 4096 at N = 20), bit for bit the round-3 answers, 102 MB of HBM traffic per launch
//     inlined against 250 MB (at 256 VGPRs there are no AGPR copies for a call boundary to save, and the call's own spills are the
//     larger traffic) and kept it inlined; the fused iteration is only trusted with the polish behind a call (lmpc_fuse_bwd below has
//     the account), and the call form alone measured 0.817 against 0.819 ms.
//   * fp32 (single precision and the fp32 pass of the mixed entry): INLINED -- the call form is 10 % slower on the mixed learning
//     kernel and changes single-precision roundings enough to lose four solves of 4096 at N = 80.
// (The switches behind these measurements went to scratch/r5/experiment_switches.patch; round 6's were removed after it.)
constexpr bool lmpc_polish_is_call(int real_bytes, int kq, int ks) { return real_bytes == 8; }

// Row-phase policies, per instantiation by measurement (profiles/r04_row_phases.md):
//   slots per chunk -- the long-horizon fp64 tracking kernels take their 11 / 14 slots half at a time (load, compute, store);
//   opaque slot tables (SlotRef, lmpc_solve_kernel.hip) -- the long-horizon fp64 kernels and every learning kernel.
// (fp32 at KQ >= 11 has no spills to begin with and loses 2-3 % to either; KQ <= 7 tracking loses 1-3 % to the opaque tables;
//  the learning kernels at KQ >= 11 lose 15 % to the chunks.)
// (bit mask of the four flag-select address sites recomputed per use in the fp64 tracking kernels with KQ <= 4: all four, -1.6..2.2 %
//  at N = 20, bit-identical; +1 % at KQ = 7 and in fp32, which keep the hoisted form: profiles/r04_row_phases.md)
__host__ __device__ constexpr int lmpc_row_chunk(int real_bytes, int kq, int ks) {
  return (real_bytes == 8 && kq >= 11 && ks == 0) ? (kq + 1) / 2 : kq;
}
__host__ __device__ constexpr bool lmpc_opaque_slots(int real_bytes, int kq, int ks) { return (real_bytes == 8 && kq >= 11) || ks > 0; }
__host__ __device__ constexpr int lmpc_opaque_sites(int real_bytes, int kq, int ks) { return (real_bytes == 8 && kq <= 4 && ks == 0) ? 15 : 0; }
// the predictor's backward sweep fused into the factorisation (riccati_factor<.., FUSE>): per instantiation, by measurement
// (MI355X, 4096 problems, kernel ms five chains -> four; profiles/r06_fuse_ab.txt):
//   fp64 tracking  N = 20 0.859 -> 0.835, N = 24 1.639 -> 1.565, N = 40 2.461 -> 2.351, N = 60 5.368 -> 4.957, IAC N = 40 4.322 -> 4.052
//   fp64 learning  N = 20 / 160 points 2.072 -> 2.028 (on); N = 40 5.52 -> 5.81, N = 60 14.54 -> 14.21 (off: KQ >= 7 with KS > 0 is the most register-starved family)
//   fp32 / mixed   IAC N = 40 3.275 -> 3.203 / 6.091 -> 5.850 (on); learning N = 20 mixed 3.385 -> 3.239, but OFF: which ill-conditioned blends
//                  of safe-set points pass the fp32 KKT test 1e-3 .. 5e-3 from the fp64 answer is decided by the last bits of the fp32
//                  sweeps -- 3 of configs[4]'s 32768 before, 5 fused (tests/test_gpu_spec_workload.py holds the 99.99 % quantile to 1e-3);
//                  tracking N <= 23 (KQ <= 4, three waves per SIMD): OFF -- the <float, 4, 0, double> instance of the fused build
//                  took a memory access fault in the mixed entry (the polish's flat store of the iterate to the save area with a
//                  clobbered address register; the fp32-array instance of the same source is fine): another of the
//                  compiler-sensitive corners of DESIGN.md section 4, found by tests/dispatch_sweep.py on its first run.
//   fp64 tracking N <= 23 (KQ <= 4, two waves per SIMD; the headline): ON, WITH THE POLISH BEHIND A CALL (lmpc_polish_is_call).  Fused with the
//                  polish inlined it gained 2.7 % and passed every test -- until an unrelated edit of the polish (a multiplier in its
//                  classification) changed the register allocation: <double, 4, 0, double> then left the iteration after its first pass
//                  (status MAX_ITER, 0 iterations; the loop's control variables read back correct; the same source with a printf, or with
//                  one more integer assigned before each break, is correct: CHANGELOG.md, round 6).  Behind a call the polish's live state
//                  (the spill source of this kernel since round 3) is out of the iteration's register allocation -- the form every
//                  one-wave kernel has always had, all of them fused without incident: 0.819 -> 0.794 ms per 4096, every GPU test green
//                  (the call form alone, unfused: 0.817).
__host__ __device__ constexpr bool lmpc_fuse_bwd(int real_bytes, int kq, int ks) {
  if (real_bytes == 8) {
    if (ks == 0) return true;  // fp64 tracking -- measured: -3 .. -8 % at every horizon (the headline with the polish behind a call)
    return kq <= 4;            // fp64 learning -- measured: N = 20 -2 %; KQ >= 7 with KS > 0, the most register-starved family, +5 % at N = 40
  }
  if (ks == 0) return kq >= 7;  // fp32 / mixed tracking -- measured: IAC N = 40 -2 / -4 %; KQ <= 4 faulted in the mixed entry when fused
  return false;                 // fp32 / mixed learning -- measured: -4 %, but 5 instead of 3 of 32768 answers past 1e-3 of the fp64 ones
}

// The stage chains on explicit LDS byte addresses (the CHAIN_PINNED form below; lmpc_solve_kernel.hip): one address per lane pattern, advanced once
// per stage, every access of the stage at a compile-time offset from one of them; the clamp of the one-stage-ahead fetch and the
// `own ? cell : junk` selects become strides of 0.  Same cells, same values, same order: only how an address is formed changes.
// On for the fp64 tracking classes of N <= 23 (KQ <= 4, KS = 0: the one-wave cold, warm and second-pass instances), whose two waves
// per SIMD share the VALU with the chain's integer work; off elsewhere (not measured there).  profiles/chain_addresses.md.
// What takes it there: the iteration's factorisation and vector solves; the active-set polish's (lmpc_polish: the plain JOSEPH
// factorisation and riccati_solve<2 | 1>); the start point's factorisation and feedback_rollout, which under the policy has the forward
// sweep's form (profiles/polish_chains.md: +1.6 % on the headline, every output bit equal).  NOT taken: the polish's first backward sweep
// fused into its factorisation -- bit equal as well, but the FUSE + JOSEPH body inside the polish's call frame costs 284 B of scratch
// per lane (672 -> 956 B in the headline kernel) and the headline 17 % (same document, section 8).
__host__ __device__ constexpr bool lmpc_chain_addr(int real_bytes, int kq, int ks) { return real_bytes == 8 && kq <= 4 && ks == 0; }

// Which instantiations keep the identity operand of the DPP reductions (lmpc_wave.hip.h: KEEP_ID).  Without it a reduction step is two
// v_mov_b32_dpp and the operation -- no identity moves, fewer hazard nops: the headline kernel loses 311 of 11 560 instructions and
// keeps its registers, scratch and spills -- and lane 63, the only lane read, has the same bits.  It is the default; kept are the
// instantiations in which the shorter form made the register allocation worse (scratch bytes or spilled VGPRs up, scratch/kinfo.py on
// the whole library: profiles/wave_reductions.md section 2):
//   fp64 learning with KQ >= 7 -- "the most register-starved family" of lmpc_fuse_bwd above -- cold and warm:
//     <7, 3> 258 -> 259 spilled VGPRs, <14, 2> 698 -> 702, <14, 3> 3384 -> 3416 B and 752 -> 781, warm <7, 2> 311 -> 325, warm <11, 3> 1064 -> 1084;
//   the two-wave kernel of KQ = 14: 836 -> 852 B, 298 -> 302.
// Every other kernel keeps or lowers both figures.  waves: wavefronts per problem.
__host__ __device__ constexpr bool lmpc_reduce_identity(int real_bytes, int kq, int ks, int waves) {
  return (real_bytes == 8 && kq >= 7 && ks > 0) || (waves == 2 && kq >= 14);
}

// ---- the three forms of a stage chain ----------------------------------------------------------------------------------------------
// The Riccati factorisation and the LDS-exchange rollout (lmpc_solve_kernel.hip) each state their stage arithmetic ONCE; the vector
// solve is one call over a fat and a lean function.  What an instantiation's form decides -- where a stage's operands are and how the
// cursor moves from stage to stage -- is described here, next to the records it walks:
//   CHAIN_INDEXED  fat records; every operand is record(i) + offset, formed at its use
//   CHAIN_PINNED   fat records; lmpc_chain_addr: one LDS byte address per lane pattern, advanced once per stage
//   CHAIN_LEAN     lean records (lmpc_lean); the stage model comes from the chunk slots of a ModelStream
// StageCells<FORM> is where the cells are and whether CHAIN_PRIO applies, CHAIN_GET / CHAIN_PUT how a cell is reached.  What the
// lean form adds to a chain -- when the chunks of the model are fetched and waited for -- stands in the bodies, under SC::lean.
enum ChainForm { CHAIN_INDEXED, CHAIN_PINNED, CHAIN_LEAN };
constexpr ChainForm lmpc_chain_form(bool lean, bool chain_addr) { return lean ? CHAIN_LEAN : (chain_addr ? CHAIN_PINNED : CHAIN_INDEXED); }

template <typename real>
struct ModelStream;  // lmpc_solve_kernel.hip
template <ChainForm FORM>
struct StageCells {
  static constexpr bool pinned = FORM == CHAIN_PINNED, lean = FORM == CHAIN_LEAN;
  // CHAIN_PRIO_* around the chain: the fat forms (where Lds::chain_prio says so); the lean chains never raise their priority
  static constexpr bool prio = !lean;
  // in the stage record L.st(i): dt, H^-1 (h00, h01 | h11), kff of right-hand side s, and K_j[c] at krow(c) + kidx + j
  static constexpr int dt = lean ? LN_DT : ST_DT, hi = lean ? LN_HI : ST_HI, hi11 = lean ? LN_HI11 : ST_HI11;
  __device__ static __forceinline__ constexpr int kff(int s) { return lean ? LN_KFF(s) : ST_KFF(s); }
  __device__ static __forceinline__ constexpr int krow(int c) { return lean ? 2 * c : ST_ROW(c); }
  static constexpr int kidx = lean ? 0 : 6;
  // in the model record of the stage (model(): the stage record itself, or the lean chunk slot): column c of [A B] as
  // six contiguous cells (c = 6, 7: the rows of B'), and g
  __device__ static __forceinline__ constexpr int row(int c) { return lean ? 6 * c : ST_ROW(c); }
  template <typename real>
  __device__ static __forceinline__ const real* model(const Lds<real>& L, const ModelStream<real>& M, int i) {
    if constexpr (lean) return M.stage(i);
    else return L.st(i);
  }
  static constexpr int g = lean ? 48 : ST_G;
};

// How a chain reaches a cell (or run of cells) that it visits in every stage.  Every access in a chain body names the cell twice over:
// as the indexed forms reach it -- record(i) + offset, formed at its use -- and by the LDS byte address `a` that the pinned form keeps
// for the lane pattern: set to the cell of the first stage, kept a register of its own from stage to stage (CHAIN_ADDR_PIN*,
// lmpc_wave.hip.h) and advanced once per stage by the record's stride, in the three blocks under SC::pinned that each chain has around
// its stage.  A store target of lanes that own nothing (a dead cell) and the clamp of the one-stage-ahead fetch are strides of 0 there.
//   CHAIN_GET(a, rec, o, k)  cell k of the run at offset o of the record: rec[o + k], or pinned lds_at(a)[k] -- a constant k is the DS
//                            instruction's immediate offset in either form
//   CHAIN_PUT(a, p, v)       *p = v (p: `own ? cell : dead cell`), or pinned *lds_at(a) = v
// What a form does not use is never evaluated.  Same cells, same values, same order in either form.  Macros (they expect the body's
// `SC` and `real`), not functions: a function boundary around an operand changes when the optimiser sees its address arithmetic, and
// with it the schedule -- the bodies are held to the device code of the separate ones they replace, instruction for instruction.
#define CHAIN_GET(a, rec, o, k) (SC::pinned ? lds_at<real>(a)[k] : (rec)[(o) + (k)])
#define CHAIN_PUT(a, p, v) do { if constexpr (SC::pinned) *lds_at<real>(a) = (v); else *(p) = (v); } while (0)

#endif
