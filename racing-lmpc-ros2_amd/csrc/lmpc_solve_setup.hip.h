// lmpc_solve_setup.hip.h -- a solve kernel's load phase: one problem's linearisation records, per-knot data and constant table from
// global memory into the LDS block, in batched reads.
// Holds: lmpc_load_problem, shared by the one-wave and the two-wave kernels (lmpc_solve_problem, under either team).
// Needs: lmpc_solve_layout.hip.h (Lds, the record offsets) and LN_DT of the lean layout (lmpc_solve_kernel.hip).
// Included by lmpc_solve_kernel.hip (all three translation units).
//
// Nothing here is on a chain, and all of it used to be waiting: the loops this replaces made one memory round trip per pass -- load,
// address arithmetic, s_waitcnt vmcnt(0), ds_write, branch -- 17 for the model at N = 20, three for the per-knot arrays, and nine
// more in the lane ladder that filled the constant table from the kernel arguments (profiles/solve_setup.md).  Here every load of
// a flight is issued before the first wait: the loads are unconditional, from an index clamped into the problem's own data (a load
// under a per-lane condition is a branch, and a branch ends the flight), the stores behind them carry the conditions.  Same values
// into the same cells as the loops: every result stays bit for bit what it was.
#ifndef LMPC_SOLVE_SETUP_HIP_H_
#define LMPC_SOLVE_SETUP_HIP_H_

#include <cstddef>

#include "lmpc_solve_layout.hip.h"

#define LMPC_LOAD_FLIGHT 20  // model loads in flight per thread at most (8-byte loads: 40 registers, and nothing else is live yet)

// the longest horizon of a slot class (lmpc_slot_class, lmpc_device.h: 64 KQ slots hold 11 N rows)
constexpr int lmpc_class_max_n(int kq) { return kq <= 2 ? 11 : (kq <= 4 ? 23 : (kq <= 7 ? 40 : (kq <= 11 ? 64 : 81))); }
// model loads per thread that bring in a whole problem of the class
constexpr int lmpc_model_loads(int kq, int threads) { return ((lmpc_class_max_n(kq) - 1) * LMPC_LIN_RECORD + threads - 1) / threads; }
constexpr int lmpc_load_chunk(int kq, int threads) {
  return lmpc_model_loads(kq, threads) < LMPC_LOAD_FLIGHT ? lmpc_model_loads(kq, threads) : LMPC_LOAD_FLIGHT;
}

// Cell c of the constant table (c = 0 .. CT_E + 5, one per thread) -> byte offset of its source in lmpc_params: selects, no table in
// memory (an indexed constexpr table would be a load of its own ahead of the one it addresses).  CT_ZERO has no source.
__device__ __forceinline__ int lmpc_ct_source(int c) {
  const int h = c - CT_HL, comp = h >> 1, lo = h & 1;  // box cells: (hi, lo) interleaved over z[0..5], u[0..1], v[0..1]
  const int box = comp < 6   ? (int)(lo ? offsetof(lmpc_params, x_min) : offsetof(lmpc_params, x_max)) + 8 * comp
                  : comp < 8 ? (int)(lo ? offsetof(lmpc_params, u_lo) : offsetof(lmpc_params, u_hi)) + 8 * (comp - 6)
                             : (int)(lo ? offsetof(lmpc_params, v_lo) : offsetof(lmpc_params, v_hi)) + 8 * (comp - 8);
  return c < CT_QT     ? (int)offsetof(lmpc_params, Qd) + 8 * (c - CT_QD)
         : c < CT_QU   ? (int)offsetof(lmpc_params, Qt) + 8 * (c - CT_QT)
         : c < CT_SV   ? (int)offsetof(lmpc_params, Qu) + 8 * (c - CT_QU)
         : c < CT_HL   ? (int)offsetof(lmpc_params, Sv) + 8 * (c - CT_SV)
         : c < CT_ZERO ? box
         : c > CT_ZERO ? (int)offsetof(lmpc_params, chs2) + 8 * (c - CT_E)
                       : (int)offsetof(lmpc_params, Qd);
}

// t: the thread's index among the THREADS that load this problem; KQ: the slot class of the instantiation, which bounds the horizon it
// is dispatched for -- and with it the model loads per thread and flight (CH), whether a single flight holds the whole record (ONE)
// and whether a thread can own more than one knot (LONG).
// LEARN: the instantiation honours P.learning (no stage cost: the one-wave kernels).  s_shift: the abscissa shift of the
// single-precision records (x_ic[0] of the problem; io(0) in fp64).  The caller closes the load with its wave / workgroup fence.
template <typename real, typename io, int THREADS, int KQ, bool LEAN, bool LEARN>
__device__ __forceinline__ void lmpc_load_problem(const lmpc_params& P, const int B, const int b, const int t, const Lds<real>& L,
                                                  const io* __restrict__ ws_lin, const io* __restrict__ x_ic, const io* __restrict__ u_ic,
                                                  const io* __restrict__ T_ref, const io* __restrict__ bl, const io* __restrict__ br,
                                                  const io* __restrict__ vref, const io s_shift) {
  constexpr int CH = lmpc_load_chunk(KQ, THREADS);
  constexpr bool ONE = lmpc_model_loads(KQ, THREADS) <= LMPC_LOAD_FLIGHT, LONG = lmpc_class_max_n(KQ) > THREADS;
  const int N = P.N, NS = N - 1;
  const real marg = real(P.marg);
  const double qv_stage = P.qv_stage, qv_term = P.qv_term;  // (both, as scalars: a select between the two fields is a load by lane)
  const bool learning = LEARN && P.learning;
  real* const ct = L.tail() + TL_CT;
  real* const KN0 = L.kn(0);

  // ---- the flight: per-knot arrays (one element per thread up to N = THREADS), initial state, one constant, the first model chunk ----
  const size_t ik = (size_t)(t < N ? t : N - 1) * B + b;
  const io v_dt = T_ref[(size_t)(t < NS ? t : NS - 1) * B + b];
  const io v_vr = vref[ik], v_bl = bl[ik], v_br = br[ik];
  const int t8 = t < 8 ? t : 7;
  const io* const p_ic = t8 < 6 ? x_ic + ((size_t)t8 * B + b) : u_ic + ((size_t)(t8 - 6) * B + b);
  const io v_ic = *p_ic;
  const int tc = t < CT_E + 6 ? t : CT_E + 5;
  const double v_ct = *reinterpret_cast<const double*>(reinterpret_cast<const char*>(&P) + lmpc_ct_source(tc));
  const int total = NS * LMPC_LIN_RECORD;
  const io* const wsb = ws_lin + (size_t)b * total;  // (every index below is clamped to total - 1: no load leaves the problem's record)
  io m[CH];
  if constexpr (!LEAN) {  // (the lean layout leaves the model in the workspace and streams it, sweep by sweep)
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int e = t + THREADS * k;
      m[k] = wsb[e < total ? e : total - 1];
    }
  }

  // ---- the stores, in the order the loads were issued ----
  if (t < NS) L.st(t)[LEAN ? LN_DT : ST_DT] = real(v_dt);
  if (t < N) {
    real* kn = L.kn(t);
    kn[KN_QLIN] = learning ? real(0) : real(t == N - 1 ? qv_term : qv_stage) * real(v_vr);
    kn[8] = 0.0;
    kn[9] = 0.0;
    kn[KN_BHL] = real(v_bl) - marg;
    kn[KN_BHL + 1] = real(v_br) + marg;
  }
  if (t < 8) KN0[t] = real(t == 0 ? v_ic - s_shift : v_ic);
  if (t < CT_E + 6) {
    // (no stage cost in the learning problem; the abscissa box moves with the abscissa: single precision carries s relative to x_ic[0])
    const bool shifted = t == CT_HL || t == CT_HL + 1;
    const real v = shifted ? real(io(v_ct) - s_shift) : real(v_ct);
    ct[t] = (t == CT_ZERO || (learning && t < CT_QU)) ? real(0) : v;
  }
  if constexpr (!LEAN) {
    // element e of the record -> stage i, cell ST_ROW(c) + k of column c = o / 6, or g[o - 48]
    auto put = [&](int e, io v) {
      const int i = e / LMPC_LIN_RECORD, o = e - i * LMPC_LIN_RECORD;
      const int c = o / 6;
      if (e < total) L.st(i)[o < 48 ? ST_ROW(c) + (o - c * 6) : ST_G + (o - 48)] = real(v);
    };
#pragma unroll
    for (int k = 0; k < CH; ++k) put(t + THREADS * k, m[k]);
    if constexpr (!ONE) {  // the longer records: further flights of CH loads
      for (int e0 = THREADS * CH; e0 < total; e0 += THREADS * CH) {
#pragma unroll
        for (int k = 0; k < CH; ++k) {
          const int e = e0 + t + THREADS * k;
          m[k] = wsb[e < total ? e : total - 1];
        }
#pragma unroll
        for (int k = 0; k < CH; ++k) put(e0 + t + THREADS * k, m[k]);
      }
    }
  }
  if constexpr (LONG) {  // horizons past one knot per thread
    for (int i = t + THREADS; i < NS; i += THREADS) L.st(i)[LEAN ? LN_DT : ST_DT] = real(T_ref[(size_t)i * B + b]);
    for (int i = t + THREADS; i < N; i += THREADS) {
      real* kn = L.kn(i);
      kn[KN_QLIN] = learning ? real(0) : real(i == N - 1 ? qv_term : qv_stage) * real(vref[(size_t)i * B + b]);
      kn[8] = 0.0;
      kn[9] = 0.0;
      kn[KN_BHL] = real(bl[(size_t)i * B + b]) - marg;
      kn[KN_BHL + 1] = real(br[(size_t)i * B + b]) + marg;
    }
  }
}

#endif
