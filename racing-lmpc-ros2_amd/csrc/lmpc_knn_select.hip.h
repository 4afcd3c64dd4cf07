// lmpc_knn_select.hip.h -- the safe-set query, once: per-lap k-nearest neighbours in (s, e_y) + cost-to-go gather, one wavefront per
// query.  lmpc_ss_query_kernel (lmpc_ss_kernel.hip: one store of laps shared by every query) and lmpc_fleet_ss_query_kernel
// (lmpc_fleet_ss_kernel.hip: each car's own ring) build a STORE POLICY and call lmpc_knn_query; what is restated, and why the scan
// is brute force, stands in lmpc_ss_kernel.hip.
//   laps newest -> oldest while fewer than S points are collected; per lap the K points of the 3n-point unrolled lap
//   [x - L e_0, x, x + L e_0] nearest to the query, nearest first (ties: lower unrolled index); J of unrolled index
//   c = rep * n + j is (n-1-j) + (1-rep)(n-1).
// One pass over a lap leaves each lane with the two nearest of its share; the 64 lane minima are sorted across the wave (bitonic
// network, lexicographic in (distance, index)) and, unless some lane's runner-up beats the take-th of them, lanes 0..take-1 hold the
// lap's neighbours nearest first and write their points in parallel.  When a lane owns two winners (a lap revisiting a place, laps
// with repeated or crawling samples) K rounds of a wave-wide arg-min pick them one at a time instead: the winner's owner retires it
// and moves on to its runner-up, or rescans its share when that is not known.
//
// A store policy provides
//   int n_laps, n                    laps to visit; the current lap's length
//   bool open(a)                     make lap a (0 = newest) current; false: nothing in it, skip
//   best2 scan(lane, Lt, qs, qe)     the best two of the lane's share of the 3n candidates (distances through lmpc_knn_dist)
//   void begin_rounds(), retire(d, i), best2 rescan(lane, Lt, qs, qe)
//                                    the rounds: forget winner (d, i) for good; the share's best two among what is left
// (scan and rescan RETURN the best two they build in locals: filled through a reference, the state reached the register allocator
// twice over -- 86 registers instead of 68 in the fleet kernel.)
//   double comp(j, k)                component k of sample j of the current lap (k = 0: before the +-L shift)
//   int code(j, rep)                 (index mode) the code of copy rep of sample j
// Every function that does arithmetic switches contraction off itself: the distance and the cost-to-go must be the same bits
// whichever kernel they are inlined into, and a file-scope pragma would reach the other kernels of the translation unit.
#ifndef LMPC_KNN_SELECT_HIP_H_
#define LMPC_KNN_SELECT_HIP_H_

#include <hip/hip_runtime.h>

#include <limits.h>

// (ad, ai) before (bd, bi), lexicographically
__device__ __forceinline__ bool lmpc_knn_less(double ad, int ai, double bd, int bi) { return ad < bd || (ad == bd && ai < bi); }

// squared distance of copy rep (0, 1, 2: at -L, 0, +L) of the point with key (ks, ke) to the query (qs, qe)
__device__ __forceinline__ double lmpc_knn_dist(double ks, double ke, int rep, double Lt, double qs, double qe) {
#pragma clang fp contract(off)
  const double s = ks + (rep - 1) * Lt;
  const double ds = s - qs, de = ke - qe;
  return ds * ds + de * de;
}

// unrolled index c = rep * n + j -> (rep, j); returns the cost-to-go J (safe_set.cpp:122,128)
__device__ __forceinline__ double lmpc_knn_point(int c, int n, int& rep, int& j) {
#pragma clang fp contract(off)
  rep = c / n;
  j = c - rep * n;
  return (double)(n - 1 - j) + (1 - rep) * (double)(n - 1);
}

// one DPP step of the arg-min.  The moves carry no identity: lanes outside ROW_MASK end the step with an unspecified pair, and the
// only lane lmpc_knn_wave_argmin reads, lane 63, is written at every one of its steps (the lane argument stands in lmpc_wave.hip.h)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void lmpc_knn_argmin_step(double& d, int& i) {
  const int od_lo = __builtin_amdgcn_mov_dpp(__double2loint(d), CTRL, ROW_MASK, 0xf, false);
  const int od_hi = __builtin_amdgcn_mov_dpp(__double2hiint(d), CTRL, ROW_MASK, 0xf, false);
  const int oi = __builtin_amdgcn_mov_dpp(i, CTRL, ROW_MASK, 0xf, false);
  const double od = __hiloint2double(od_hi, od_lo);
  if (lmpc_knn_less(od, oi, d, i)) {
    d = od;
    i = oi;
  }
}

// wave-wide lexicographic arg-min of (distance, unrolled index) on the VALU: four row_ror steps give every lane of a 16-lane row
// the row's winner, row_bcast15 / row_bcast31 fold the rows into lane 63, which every lane then reads
__device__ __forceinline__ void lmpc_knn_wave_argmin(double& d, int& i) {
  lmpc_knn_argmin_step<0x128, 0xf>(d, i);
  lmpc_knn_argmin_step<0x124, 0xf>(d, i);
  lmpc_knn_argmin_step<0x122, 0xf>(d, i);
  lmpc_knn_argmin_step<0x121, 0xf>(d, i);
  lmpc_knn_argmin_step<0x142, 0xa>(d, i);
  lmpc_knn_argmin_step<0x143, 0xc>(d, i);
  d = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(d), 63), __builtin_amdgcn_readlane(__double2loint(d), 63));
  i = __builtin_amdgcn_readlane(i, 63);
}

// the 64 lanes' (d, i) sorted ascending across the wave: bitonic network, lexicographic in (distance, index)
__device__ __forceinline__ void lmpc_knn_sort64(double& d, int& i, int lane) {
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      const double od = __shfl_xor(d, jj, 64);
      const int oi = __shfl_xor(i, jj, 64);
      const bool other_less = lmpc_knn_less(od, oi, d, i);
      const bool keep_min = ((lane & jj) == 0) == ((lane & k) == 0);
      if (keep_min ? other_less : !other_less) {
        d = od;
        i = oi;
      }
    }
  }
}

// The two nearest candidates of a lane's share.  Neighbours are close in index and a share is strided by 64, so a lane seldom owns
// more than one of the K winners: its runner-up is promoted without another pass.
// seci is a three-state flag: an index, INT_MAX = the share has no further candidate, -1 = not known (rescan).
struct lmpc_knn_best2 {
  double bestd, secd;
  int besti, seci;
  __device__ __forceinline__ void clear() {
    bestd = secd = INFINITY;
    besti = seci = INT_MAX;
  }
  // IN_ORDER: the caller's candidates arrive by increasing index, so a strict < already keeps the lower index of a tie.  The
  // shared-store scan and its LDS rescan are such callers and keep this cheaper rule: on in-order arrivals both rules give the same
  // best two, and with the full rule the scan loop compiles to 303 instructions per trip of four points instead of 196, the LDS
  // rescan to 55 instead of 30.
  // Otherwise the full lexicographic rule; +inf and NaN never enter (INT_MAX = no candidate).
  template <bool IN_ORDER>
  __device__ __forceinline__ void enter(double d, int c) {
    if (d < bestd || (!IN_ORDER && d == bestd && c < besti && d < INFINITY)) {
      secd = bestd;
      seci = besti;
      bestd = d;
      besti = c;
    } else if (d < secd || (!IN_ORDER && d == secd && c < seci && d < INFINITY)) {
      secd = d;
      seci = c;
    }
  }
  // the best has been taken: its runner-up moves up.  false when the runner-up is not known: rescan.
  __device__ __forceinline__ bool promote() {
    if (seci < 0) return false;
    bestd = secd;
    besti = seci;
    secd = INFINITY;
    seci = besti == INT_MAX ? INT_MAX : -1;
    return true;
  }
};

// Fast path: with the lane minima sorted and (td, ti) the take-th of them, the first `take` lanes hold the lap's neighbours unless
// some lane's runner-up beats (td, ti) -- or fewer than `take` finite distances exist (a NaN query)
__device__ __forceinline__ bool lmpc_knn_fast_path_ok(const lmpc_knn_best2& m, double td, int ti) {
  const bool beaten = m.seci != INT_MAX && lmpc_knn_less(m.secd, m.seci, td, ti);
  return !__any(beaten) && ti != INT_MAX;
}

// Pad with the last point (racing_mpc.cpp:263-272): `last` holds component k on lane k < 6 and J - J0 on lane 6.
__device__ __forceinline__ void lmpc_knn_pad(int tot, int S, int B, int b, int lane, double last, double* __restrict__ ss_x,
                                             double* __restrict__ ss_j) {
  for (int q = tot; q < S; ++q) {
    if (lane < 6)
      ss_x[((size_t)lane * S + q) * B + b] = last;
    else if (lane == 6)
      ss_j[(size_t)q * B + b] = last;
  }
}

// The query of problem b on `lane` of its wavefront.  Out: ss_x [6][S][B], ss_j [S][B] (J - J0), n_found [B]; j0_out (may be null):
// the cost-to-go of the first point, subtracted from ss_j (racing_mpc.cpp:280).
// Index mode (ss_idx != null): instead of the 7 S doubles a query leaves S int32 codes, st.code of the points; -1: no point.
template <class Store>
__device__ __forceinline__ void lmpc_knn_query(Store& st, int B, int b, int lane, int S, int K, double Lt, const double* __restrict__ query,
                                               double* __restrict__ ss_x, double* __restrict__ ss_j, int* __restrict__ n_found,
                                               double* __restrict__ j0_out, int* __restrict__ ss_idx) {
#pragma clang fp contract(off)
  const double qs = query[b], qe = query[(size_t)B + b];
  int tot = 0;
  double last = 0.0;  // lane k < 6: component k of the last point written; lane 6: its J - J0
  double j0 = 0.0;
  int last_code = -1;  // (index mode) the code of the last point taken: what the padding repeats
  for (int a = 0; a < st.n_laps && tot < S; ++a) {  // newest lap first
    if (!st.open(a)) continue;
    const int n = st.n, n3 = 3 * n;
    lmpc_knn_best2 m = st.scan(lane, Lt, qs, qe);
    int take = K < n3 ? K : n3;
    if (take > S - tot) take = S - tot;
    if (take <= 64) {
      double d = m.bestd;
      int i = m.besti;
      lmpc_knn_sort64(d, i, lane);
      const double td = __shfl(d, take - 1, 64);
      const int ti = __shfl(i, take - 1, 64);
      if (lmpc_knn_fast_path_ok(m, td, ti)) {  // every lane writes its own point
        const bool mine = lane < take;
        int rep, j;
        const double jv = lmpc_knn_point(mine ? i : 0, n, rep, j);
        if (tot == 0) j0 = __shfl(jv, 0, 64);
        if (mine) {
          if (ss_idx) {
            ss_idx[(size_t)(tot + lane) * B + b] = st.code(j, rep);
          } else {
#pragma unroll
            for (int k = 0; k < 6; ++k) ss_x[((size_t)k * S + tot + lane) * B + b] = st.comp(j, k) + (k == 0 ? (rep - 1) * Lt : 0.0);
            ss_j[(size_t)(tot + lane) * B + b] = jv - j0;
          }
        }
        // the last point written, as the padding wants it
        int repl, jl;
        const double jvl = lmpc_knn_point(ti, n, repl, jl);
        if (lane < 6)
          last = st.comp(jl, lane) + (lane == 0 ? (repl - 1) * Lt : 0.0);
        else if (lane == 6)
          last = jvl - j0;
        last_code = st.code(jl, repl);
        tot += take;
        continue;
      }
    }
    st.begin_rounds();
    for (int q = 0; q < take; ++q, ++tot) {
      double d = m.bestd;
      int i = m.besti;
      lmpc_knn_wave_argmin(d, i);
      if (i == INT_MAX) break;  // no finite distance left (a NaN query from a diverged car state): nothing more to take
      int rep, j;
      const double jv = lmpc_knn_point(i, n, rep, j);
      if (tot == 0) j0 = jv;
      last_code = st.code(j, rep);
      if (ss_idx) {
        if (lane == 0) ss_idx[(size_t)tot * B + b] = last_code;
      } else if (lane < 6) {
        last = st.comp(j, lane) + (lane == 0 ? (rep - 1) * Lt : 0.0);
        ss_x[((size_t)lane * S + tot) * B + b] = last;
      } else if (lane == 6) {
        last = jv - j0;
        ss_j[(size_t)tot * B + b] = last;
      }
      if (m.besti == i) {  // the winner's owner retires it and moves on to its runner-up
        st.retire(m.bestd, i);
        if (!m.promote()) m = st.rescan(lane, Lt, qs, qe);  // second win in a row without a known runner-up
      }
    }
  }
  if (lane == 0) {
    n_found[b] = tot;
    if (j0_out) j0_out[b] = j0;
  }
  // With nothing found (no lap stored, or a NaN query) the reference keeps its previous parameter values; a batch has no
  // "previous", so the outputs are zero-filled -- defined data -- and n_found = 0 tells the caller not to solve on them.
  if (tot == 0) last = 0.0;
  if (ss_idx) {
    for (int q = tot + lane; q < S; q += 64) ss_idx[(size_t)q * B + b] = last_code;
    return;
  }
  lmpc_knn_pad(tot, S, B, b, lane, last, ss_x, ss_j);
}

#endif  // LMPC_KNN_SELECT_HIP_H_
