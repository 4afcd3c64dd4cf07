// lmpc_fleet_ss_kernel.hip -- the fleet safe set on gfx950: SafeSetRecorder::step for every car in one launch, and the k-NN
// query of lmpc_ss_kernel.hip against each car's OWN ring of laps.  Layout: lmpc_fleet_ss.h.
//
// Query: one wavefront per car, as in the shared-store kernel, with the same selection (per-lane best two, 64-lane bitonic sort
// lexicographic in (distance, unrolled index), K arg-min rounds when a lane owns two winners) and the same distance expression
// in the same order, so that on equal stores the results are bit-equal.  What differs is where the bytes come from: a car's
// keys are nobody else's, so they come from HBM and are read ONCE --
//   - a lane reads the 16-byte key of sample j and derives the three unrolled candidates (j, n + j, 2n + j: the copies at -L, 0,
//     +L) arithmetically, instead of visiting 3n rows of [n][6];
//   - eight independent 16-byte loads per lane are issued before the first is used (8 KB in flight per wave: one trip covers a
//     lap of 512 samples), against ~900 cycles of HBM latency;
//   - NO LDS: the shared-store kernel keeps all 3n distances in LDS for its rare rescan, sized by the longest stored lap, which
//     for a fleet the host does not know (the capacity would cost 24 KB per wave and cap a CU at six waves).  Here the rescan
//     RECOMPUTES the distances from the keys.  Which candidates of a lane's share are already taken needs no bit mask either:
//     winners leave in increasing (distance, index) order, so a lane's retired candidates are exactly those of its share not
//     above the last one it gave up -- one (distance, index) threshold per lane.  Waves per CU are bounded by registers alone.
// A lane's candidates do not come in index order (j ascending, rep inside), so its best two are kept by the full lexicographic
// comparison rather than by arrival.
#include <hip/hip_runtime.h>

#include <limits.h>

#include "lmpc_fleet_ss.h"

// ---- recorder: SafeSetRecorder::step (safe_set.cpp:278-322) + SafeSetManager::add_lap (:144-151), one thread per car ----
__global__ __launch_bounds__(256) void lmpc_fleet_ss_record_kernel(lmpc_fleet_store st, const double* __restrict__ x,
                                                                   const double* __restrict__ u, const double* __restrict__ k, double t,
                                                                   double Lt, const int* __restrict__ active) {
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x), B = st.B;
  if (b >= B) return;
  if (active && active[b] == 0) return;
  const double s = x[b];
  int fl = st.flags[b];
  if (!(fl & LMPC_FLEET_FLAG_VALID)) {  // the very first sample only seeds the abscissa (:278-282)
    st.s_prev[b] = s;
    st.flags[b] = fl | LMPC_FLEET_FLAG_VALID;
    return;
  }
  const double sp = st.s_prev[b];
  st.s_prev[b] = s;
  const int R1 = st.R + 1, C = st.C;
  int head = st.head[b], at = -1;
  if (sp - s > 0.5 * Lt) {  // crossed the start line
    if (fl & LMPC_FLEET_FLAG_INIT) {
      const size_t slot = (size_t)b * R1 + head;
      const int dn = st.dur_n[b];
      st.dur[(size_t)b * LMPC_FLEET_DUR + dn % LMPC_FLEET_DUR] = t - st.aux[slot * C * 4 + 3];  // t at the crossing - t of the lap's first sample
      st.dur_n[b] = dn + 1;
      if (fl & LMPC_FLEET_FLAG_OVERFLOW) {  // longer than a slot: not added, nothing evicted; the slot is reused for the next lap
        st.n_dropped[b] += 1;
      } else {  // the open lap becomes the newest of the ring where it stands; the next slot (unused, or the oldest lap) opens
        st.npts[slot] = st.open_n[b];
        head = head + 1 == R1 ? 0 : head + 1;
        st.head[b] = head;
        const int c = st.cnt[b];
        if (c < st.R) st.cnt[b] = c + 1;
      }
    }  // else: the first, partial lap is discarded (:296-300)
    st.flags[b] = (fl | LMPC_FLEET_FLAG_INIT) & ~LMPC_FLEET_FLAG_OVERFLOW;
    st.lap_count[b] += 1;
    st.open_n[b] = 1;  // the closing sample starts the next lap
    at = 0;
  } else if (fl & LMPC_FLEET_FLAG_INIT) {
    const int n = st.open_n[b];
    if (n < C) {
      at = n;
      st.open_n[b] = n + 1;
    } else if (!(fl & LMPC_FLEET_FLAG_OVERFLOW)) {  // the slot is full: the lap stops storing and will be dropped at its close
      st.flags[b] = fl | LMPC_FLEET_FLAG_OVERFLOW;
    }
  }
  if (at < 0) return;
  const size_t row = ((size_t)b * R1 + head) * C + at;  // at < C, head <= R: inside car b's slots
  st.key[row] = make_double2(s, x[(size_t)B + b]);
  double* xr = st.xr + row * 4;
  double* ax = st.aux + row * 4;
#pragma unroll
  for (int c = 0; c < 4; ++c) xr[c] = x[(size_t)(2 + c) * B + b];
  ax[0] = u[b];
  ax[1] = u[(size_t)B + b];
  ax[2] = k[b];
  ax[3] = t;
}

// ---- SafeSetRecorder::load (safe_set.cpp:260-276) for one car (grid 1) or every car (grid B): one workgroup per car pushes
// n_laps staged laps (host-trimmed to the ring's size, each <= C samples) into the ring.  The open lap stands in the slot a new
// lap must take, so it moves one slot on first. ----
__global__ __launch_bounds__(256) void lmpc_fleet_ss_load_kernel(lmpc_fleet_store st, int car, int n_laps, const int* __restrict__ lap_n,
                                                                 const int* __restrict__ lap_off, const double* __restrict__ x,
                                                                 const double* __restrict__ u, const double* __restrict__ k,
                                                                 const double* __restrict__ t) {
  const int b = car < 0 ? (int)blockIdx.x : car;
  if (b >= st.B) return;
  const int R1 = st.R + 1, C = st.C, tid = threadIdx.x;
  for (int l = 0; l < n_laps; ++l) {
    const int head = st.head[b], nh = head + 1 == R1 ? 0 : head + 1;
    const int on = (st.flags[b] & LMPC_FLEET_FLAG_INIT) ? st.open_n[b] : 0;
    const size_t r0 = ((size_t)b * R1 + head) * C, r1 = ((size_t)b * R1 + nh) * C;
    for (int i = tid; i < on && i < C; i += 256) {
      st.key[r1 + i] = st.key[r0 + i];
      for (int c = 0; c < 4; ++c) {
        st.xr[(r1 + i) * 4 + c] = st.xr[(r0 + i) * 4 + c];
        st.aux[(r1 + i) * 4 + c] = st.aux[(r0 + i) * 4 + c];
      }
    }
    __syncthreads();
    const int n = lap_n[l] < C ? lap_n[l] : C;
    const size_t o = (size_t)lap_off[l];
    for (int i = tid; i < n; i += 256) {
      st.key[r0 + i] = make_double2(x[(o + i) * 6], x[(o + i) * 6 + 1]);
      for (int c = 0; c < 4; ++c) st.xr[(r0 + i) * 4 + c] = x[(o + i) * 6 + 2 + c];
      st.aux[(r0 + i) * 4] = u[(o + i) * 2];
      st.aux[(r0 + i) * 4 + 1] = u[(o + i) * 2 + 1];
      st.aux[(r0 + i) * 4 + 2] = k[o + i];
      st.aux[(r0 + i) * 4 + 3] = t[o + i];
    }
    __syncthreads();
    if (tid == 0) {
      st.npts[(size_t)b * R1 + head] = n;
      st.head[b] = nh;
      const int c = st.cnt[b];
      if (c < st.R) st.cnt[b] = c + 1;
      st.lap_count[b] += 1;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void lmpc_fleet_ss_stats_kernel(lmpc_fleet_store st, int* __restrict__ laps_in_ring,
                                                                  int* __restrict__ lap_count, int* __restrict__ n_dropped,
                                                                  double* __restrict__ last_lap_time) {
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b >= st.B) return;
  if (laps_in_ring) laps_in_ring[b] = st.cnt[b];
  if (lap_count) lap_count[b] = st.lap_count[b];
  if (n_dropped) n_dropped[b] = st.n_dropped[b];
  if (last_lap_time) {
    const int dn = st.dur_n[b];
    last_lap_time[b] = dn > 0 ? st.dur[(size_t)b * LMPC_FLEET_DUR + (dn - 1) % LMPC_FLEET_DUR] : 0.0;
  }
}

// one DPP step of the wave-wide arg-min (as in lmpc_ss_kernel.hip): lanes outside ROW_MASK see the identity (+inf, INT_MAX)
#define FLEET_ARGMIN_STEP(CTRL, ROW_MASK)                                                                                \
  {                                                                                                                      \
    const int od_lo = __builtin_amdgcn_update_dpp(0, __double2loint(d), CTRL, ROW_MASK, 0xf, false);                     \
    const int od_hi = __builtin_amdgcn_update_dpp(0x7ff00000, __double2hiint(d), CTRL, ROW_MASK, 0xf, false);            \
    const int oi = __builtin_amdgcn_update_dpp(INT_MAX, i, CTRL, ROW_MASK, 0xf, false);                                  \
    const double od = __hiloint2double(od_hi, od_lo);                                                                    \
    if (od < d || (od == d && oi < i)) {                                                                                 \
      d = od;                                                                                                            \
      i = oi;                                                                                                            \
    }                                                                                                                    \
  }

// the three unrolled candidates of key (ks, ke), sample j of a lap of n: the distance expression of lmpc_ss_query_kernel, operation
// for operation; a candidate enters the lane's best two by (distance, index), +inf and NaN never do (INT_MAX = no candidate)
#define FLEET_CANDIDATES(KS, KE, J, FILTER)                                                                              \
  _Pragma("unroll") for (int rep = 0; rep < 3; ++rep) {                                                                  \
    const double s = (KS) + (rep - 1) * Lt;                                                                              \
    const double ds = s - qs, de = (KE) - qe;                                                                            \
    const double d = ds * ds + de * de;                                                                                  \
    const int c = rep * n + (J);                                                                                         \
    if (FILTER) {                                                                                                        \
      if (d < bestd || (d == bestd && c < besti && d < INFINITY)) {                                                      \
        secd = bestd;                                                                                                    \
        seci = besti;                                                                                                    \
        bestd = d;                                                                                                       \
        besti = c;                                                                                                       \
      } else if (d < secd || (d == secd && c < seci && d < INFINITY)) {                                                  \
        secd = d;                                                                                                        \
        seci = c;                                                                                                        \
      }                                                                                                                  \
    }                                                                                                                    \
  }

__global__ __launch_bounds__(64) void lmpc_fleet_ss_query_kernel(lmpc_fleet_store st, int S, int K, double Lt,
                                                                 const double* __restrict__ query, double* __restrict__ ss_x,
                                                                 double* __restrict__ ss_j, int* __restrict__ n_found) {
#pragma clang fp contract(off)
  // XCD-aware assignment, as in lmpc_ss_query_kernel: the 8-byte results of neighbouring cars share 64-byte lines of the
  // [field][point][batch] arrays and are merged in one XCD's L2
  const int B = st.B;
  const int b = (int)(blockIdx.x & 7) * ((B + 7) >> 3) + (int)(blockIdx.x >> 3), lane = threadIdx.x;
  if (b >= B) return;
  const double qs = query[b], qe = query[(size_t)B + b];
  const int R1 = st.R + 1, C = st.C;
  const int head = st.head[b], cnt = st.cnt[b] < st.R ? st.cnt[b] : st.R;
  int tot = 0;
  double last = 0.0;  // lane k < 6: component k of the last point written; lane 6: its J - J0
  double j0 = 0.0;
  for (int a = 0; a < cnt && tot < S; ++a) {  // newest lap first
    int sl = head - 1 - a;
    if (sl < 0) sl += R1;
    const size_t slot = (size_t)b * R1 + sl;
    int n = st.npts[slot];
    if (n > C) n = C;
    if (n < 1) continue;
    const int n3 = 3 * n;
    const double2* __restrict__ kl = st.key + slot * C;
    const double* __restrict__ xl = st.xr + slot * C * 4;
    double bestd = INFINITY, secd = INFINITY;
    int besti = INT_MAX, seci = INT_MAX;  // seci: INT_MAX = the share has no further candidate, -1 = not known (rescan)
    for (int base = 0; base < n; base += 512) {
      double2 kv[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int j = base + lane + 64 * t;
        kv[t] = kl[j < n ? j : 0];
      }
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int j = base + lane + 64 * t;
        if (j < n) { FLEET_CANDIDATES(kv[t].x, kv[t].y, j, true) }
      }
    }
    int take = K < n3 ? K : n3;
    if (take > S - tot) take = S - tot;
    // Fast path: the 64 lane minima sorted across the wave; valid unless some lane's runner-up beats the take-th of them
    if (take <= 64) {
      double d = bestd;
      int i = besti;
#pragma unroll
      for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
          const double od = __shfl_xor(d, jj, 64);
          const int oi = __shfl_xor(i, jj, 64);
          const bool other_less = od < d || (od == d && oi < i);
          const bool keep_min = ((lane & jj) == 0) == ((lane & k) == 0);
          if (keep_min ? other_less : !other_less) {
            d = od;
            i = oi;
          }
        }
      }
      const double td = __shfl(d, take - 1, 64);
      const int ti = __shfl(i, take - 1, 64);
      const bool beaten = seci != INT_MAX && (secd < td || (secd == td && seci < ti));
      if (!__any(beaten) && ti != INT_MAX) {
        const bool mine = lane < take;
        const int ii = mine ? i : 0;
        const int rep = ii / n, j = ii - rep * n;
        const double jv = (double)(n - 1 - j) + (1 - rep) * (double)(n - 1);
        if (tot == 0) j0 = __shfl(jv, 0, 64);
        if (mine) {
          const double2 kp = kl[j];
          const size_t o = (size_t)(tot + lane) * B + b, SB = (size_t)S * B;
          ss_x[o] = kp.x + (rep - 1) * Lt;
          ss_x[SB + o] = kp.y + 0.0;
#pragma unroll
          for (int k = 0; k < 4; ++k) ss_x[(size_t)(k + 2) * SB + o] = xl[(size_t)j * 4 + k] + 0.0;
          ss_j[o] = jv - j0;
        }
        // the last point written, as the padding below wants it: component k on lane k < 6, J - J0 on lane 6
        const int il = __shfl(i, take - 1, 64);
        const int repl = il / n, jl = il - repl * n;
        if (lane == 0)
          last = kl[jl].x + (repl - 1) * Lt;
        else if (lane == 1)
          last = kl[jl].y + 0.0;
        else if (lane < 6)
          last = xl[(size_t)jl * 4 + lane - 2] + 0.0;
        else if (lane == 6)
          last = ((double)(n - 1 - jl) + (1 - repl) * (double)(n - 1)) - j0;
        tot += take;
        continue;
      }
    }
    double thd = 0.0;  // the last candidate this lane gave up: everything of its share up to it, by (distance, index), is taken
    int thi = -1;
    for (int q = 0; q < take; ++q, ++tot) {
      double d = bestd;
      int i = besti;
      FLEET_ARGMIN_STEP(0x128, 0xf)
      FLEET_ARGMIN_STEP(0x124, 0xf)
      FLEET_ARGMIN_STEP(0x122, 0xf)
      FLEET_ARGMIN_STEP(0x121, 0xf)
      FLEET_ARGMIN_STEP(0x142, 0xa)
      FLEET_ARGMIN_STEP(0x143, 0xc)
      d = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(d), 63), __builtin_amdgcn_readlane(__double2loint(d), 63));
      i = __builtin_amdgcn_readlane(i, 63);
      if (i == INT_MAX) break;  // no finite distance left (a NaN query): nothing more to take
      const int rep = i / n, j = i - rep * n;
      const double jv = (double)(n - 1 - j) + (1 - rep) * (double)(n - 1);
      if (tot == 0) j0 = jv;
      if (lane < 6) {
        if (lane == 0)
          last = kl[j].x + (rep - 1) * Lt;
        else if (lane == 1)
          last = kl[j].y + 0.0;
        else
          last = xl[(size_t)j * 4 + lane - 2] + 0.0;
        ss_x[((size_t)lane * S + tot) * B + b] = last;
      } else if (lane == 6) {
        last = jv - j0;
        ss_j[(size_t)tot * B + b] = last;
      }
      if (besti == i) {  // the winner's owner retires it and moves on to its runner-up
        thd = bestd;
        thi = besti;
        if (seci >= 0) {
          bestd = secd;
          besti = seci;
          secd = INFINITY;
          seci = besti == INT_MAX ? INT_MAX : -1;
        } else {  // second win in a row without a known runner-up: the share's two smallest above the threshold, from the keys
          bestd = secd = INFINITY;
          besti = seci = INT_MAX;
          for (int jr = lane; jr < n; jr += 64) {
            const double2 kp = kl[jr];
            FLEET_CANDIDATES(kp.x, kp.y, jr, (d > thd || (d == thd && c > thi)))
          }
        }
      }
    }
  }
  if (lane == 0) n_found[b] = tot;
  // pad with the last point (racing_mpc.cpp:263-272); nothing found (an empty ring, a NaN query): zero-filled, n_found = 0
  if (tot == 0) last = 0.0;
  for (int q = tot; q < S; ++q) {
    if (lane < 6)
      ss_x[((size_t)lane * S + q) * B + b] = last;
    else if (lane == 6)
      ss_j[(size_t)q * B + b] = last;
  }
}
