// lmpc_fleet_ss_kernel.hip -- the fleet safe set on gfx950: SafeSetRecorder::step for every car in one launch, and the k-NN
// query of lmpc_ss_kernel.hip against each car's OWN ring of laps.  Layout: lmpc_fleet_ss.h.
//
// Query: one wavefront per car; the selection is lmpc_knn_select.hip.h, the one the shared-store kernel runs, so on equal stores the
// results are bit-equal.  This file holds the store behind it, a car's ring.  What differs from the shared store is where the bytes
// come from: a car's keys are nobody else's, so they come from HBM and are read ONCE --
//   - a lane reads the 16-byte key of sample j and derives the three unrolled candidates (j, n + j, 2n + j: the copies at -L, 0,
//     +L) arithmetically, instead of visiting 3n rows of [n][6];
//   - eight independent 16-byte loads per lane are issued before the first is used (8 KB in flight per wave: one trip covers a
//     lap of 512 samples), against ~900 cycles of HBM latency;
//   - NO LDS: the shared-store kernel keeps all 3n distances in LDS for its rare rescan, sized by the longest stored lap, which
//     for a fleet the host does not know (the capacity would cost 24 KB per wave and cap a CU at six waves).  Here the rescan
//     RECOMPUTES the distances from the keys.  Which candidates of a lane's share are already taken needs no bit mask either:
//     winners leave in increasing (distance, index) order, so a lane's retired candidates are exactly those of its share not
//     above the last one it gave up -- one (distance, index) threshold per lane.  Waves per CU are bounded by registers alone.
#include <hip/hip_runtime.h>

#include <limits.h>

#include "lmpc_fleet_ss.h"
#include "lmpc_knn_select.hip.h"
#include "lmpc_loop_steps.hip.h"  // lmpc_fleet_record_car: the recorder's step, shared with lmpc_fleet_loop_kernel.hip

// ---- recorder: SafeSetRecorder::step (safe_set.cpp:278-322) + SafeSetManager::add_lap (:144-151), one thread per car ----
__global__ __launch_bounds__(256) void lmpc_fleet_ss_record_kernel(lmpc_fleet_store st, const double* __restrict__ x,
                                                                   const double* __restrict__ u, const double* __restrict__ k, double t,
                                                                   double Lt, const int* __restrict__ active) {
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x), B = st.B;
  if (b >= B) return;
  if (active && active[b] == 0) return;
  double xs[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) xs[c] = x[(size_t)c * B + b];
  lmpc_fleet_record_car(st, b, xs, u[b], u[(size_t)B + b], k[b], t, Lt);
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

// A car's ring of laps as the store of lmpc_knn_query.
struct lmpc_ss_fleet_ring {
  int n_laps;  // laps in the ring, clamped to its size
  const lmpc_fleet_store& st;
  int b, head, n;
  const double2* __restrict__ kl;  // the current lap: keys (s, e_y), and the other four components
  const double* __restrict__ xl;
  double thd;  // the last candidate this lane gave up: everything of its share up to it, by (distance, index), is taken
  int thi;
  __device__ __forceinline__ bool open(int a) {
    const int R1 = st.R + 1, C = st.C;
    int sl = head - 1 - a;
    if (sl < 0) sl += R1;
    const size_t slot = (size_t)b * R1 + sl;
    kl = st.key + slot * C;
    xl = st.xr + slot * C * 4;
    n = st.npts[slot];
    if (n > C) n = C;
    return n >= 1;
  }
  // the three unrolled candidates of key kp, sample j of a lap of n (j, n + j, 2n + j: the copies at -L, 0, +L).  They do not come
  // in index order (j ascending, rep inside), so they enter by the full lexicographic rule.  FILTERED: only those above the threshold.
  template <bool FILTERED>
  __device__ __forceinline__ void candidates(lmpc_knn_best2& m, double2 kp, int j, double Lt, double qs, double qe) const {
#pragma unroll
    for (int rep = 0; rep < 3; ++rep) {
      const double d = lmpc_knn_dist(kp.x, kp.y, rep, Lt, qs, qe);
      const int c = rep * n + j;
      if (!FILTERED || d > thd || (d == thd && c > thi)) m.enter<false>(d, c);
    }
  }
  // eight independent 16-byte loads per lane are issued before the first is used (8 KB in flight per wave: one trip covers a lap of
  // 512 samples), against ~900 cycles of HBM latency
  __device__ __forceinline__ lmpc_knn_best2 scan(int lane, double Lt, double qs, double qe) const {
    lmpc_knn_best2 m;
    m.clear();
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
        if (j < n) candidates<false>(m, kv[t], j, Lt, qs, qe);
      }
    }
    return m;
  }
  __device__ __forceinline__ void begin_rounds() {
    thd = 0.0;
    thi = -1;
  }
  __device__ __forceinline__ void retire(double d, int i) {
    thd = d;
    thi = i;
  }
  // the share's two smallest above the threshold, from the keys
  __device__ __forceinline__ lmpc_knn_best2 rescan(int lane, double Lt, double qs, double qe) const {
    lmpc_knn_best2 m;
    m.clear();
    for (int jr = lane; jr < n; jr += 64) candidates<true>(m, kl[jr], jr, Lt, qs, qe);
    return m;
  }
  __device__ __forceinline__ double comp(int j, int k) const { return k == 0 ? kl[j].x : (k == 1 ? kl[j].y : xl[(size_t)j * 4 + k - 2]); }
  __device__ __forceinline__ int code(int, int) const { return -1; }  // (no index mode on a ring)
};

__global__ __launch_bounds__(64) void lmpc_fleet_ss_query_kernel(lmpc_fleet_store st, int S, int K, double Lt,
                                                                 const double* __restrict__ query, double* __restrict__ ss_x,
                                                                 double* __restrict__ ss_j, int* __restrict__ n_found) {
  // XCD-aware assignment, as in lmpc_ss_query_kernel: the 8-byte results of neighbouring cars share 64-byte lines of the
  // [field][point][batch] arrays and are merged in one XCD's L2
  const int B = st.B;
  const int b = (int)(blockIdx.x & 7) * ((B + 7) >> 3) + (int)(blockIdx.x >> 3), lane = threadIdx.x;
  if (b >= B) return;
  lmpc_ss_fleet_ring ring{st.cnt[b] < st.R ? st.cnt[b] : st.R, st, b, st.head[b], 0, nullptr, nullptr, 0.0, -1};
  lmpc_knn_query(ring, B, b, lane, S, K, Lt, query, ss_x, ss_j, n_found, nullptr, nullptr);
}
