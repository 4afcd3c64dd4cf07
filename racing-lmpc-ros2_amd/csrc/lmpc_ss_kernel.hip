// lmpc_ss_kernel.hip -- LMPC safe-set query on gfx950: per-lap k-nearest neighbours in (s, e_y)
// + cost-to-go gather.  One wavefront per query.
//
// Restates SafeSetManager::query(SSQuery) (safe_set.cpp:153-180) over SSTrajectory::query
// (:42-54) and TrajectoryKDTree::find_closest_waypoint_indices (trajectory_kd_tree.cpp:53-63),
// with the +-L unrolling and cost-to-go of SSTrajectory::process_lap_data (:116-137) done
// arithmetically instead of being stored, and the pad / truncate / J - J[0] post-processing of
// RacingMPC::solve (racing_mpc.cpp:263-280) fused in.
// Index mode (ss_idx != NULL, round 5): instead of the 7 S doubles of (ss_x, ss_j) a query leaves S int32 codes
//   code = ((row of the point in the concatenated lap store) << 2) | rep        (rep = 0, 1, 2: the -L, 0, +L copy; -1: no point)
// and the learning kernel's prologue gathers the points from the L2-resident store itself (lmpc_solve_kernel.hip): 640 B per
// query instead of 8960 B written here and read back there, and 4-byte stores that merge 16 to a line instead of 8.
// The selection itself (per-lane best two, 64-lane bitonic sort, K arg-min rounds when a lane owns two winners; ties: lower unrolled
// index -- CGAL's order for exact ties is unspecified) is lmpc_knn_select.hip.h, shared with the fleet kernel; this file holds the
// shared store behind it.  The brute-force scan replaces CGAL's kd-tree: one pass over the 3n unrolled points of a lap leaves each
// lane with the two nearest of its strided share, all distances staying in LDS.
#include <hip/hip_runtime.h>

#include "lmpc_knn_select.hip.h"

// The shared store: laps concatenated as x [sum n][6], lap l at row off[l] with npts[l] samples; every query reads the same laps, so
// they come from L2.  All 3n distances of the current lap stay in LDS (dist, sized by the longest lap) for the rare rescan.
struct lmpc_ss_shared_store {
  int n_laps;
  const int* __restrict__ npts;
  const int* __restrict__ off;
  const double* __restrict__ x;
  double* dist;
  const double* xl;  // the current lap
  int offl, n;
  __device__ __forceinline__ bool open(int a) {
    const int l = n_laps - 1 - a;
    n = npts[l];
    offl = off[l];
    xl = x + (size_t)offl * 6;
    __syncthreads();  // dist is reused
    return true;      // (lmpc_set_safe_set refuses an empty lap)
  }
  // one pass: distance of every unrolled point of the lane's strided share, kept in LDS, and the share's two smallest in registers.
  // four points of the share per trip, their loads issued together (one point per trip left the pass waiting on a dependent
  // L2 round trip per point, behind an integer division for (rep, j): 62 us per query wave), (rep, j) stepped, not divided
  __device__ __forceinline__ lmpc_knn_best2 scan(int lane, double Lt, double qs, double qe) {
    lmpc_knn_best2 m;
    m.clear();
    const int n3 = 3 * n;
    int j = lane, rep = 0;
    while (j >= n) {
      j -= n;
      ++rep;
    }
    for (int c = lane; c < n3; c += 256) {
      double sv[4], ev[4];
      int rp[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const bool in = c + 64 * t < n3;
        const int jj = in ? j : 0;
        sv[t] = xl[(size_t)jj * 6];
        ev[t] = xl[(size_t)jj * 6 + 1];
        rp[t] = rep;
        j += 64;
        while (j >= n) {
          j -= n;
          ++rep;
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int ct = c + 64 * t;
        if (ct < n3) {
          const double d = lmpc_knn_dist(sv[t], ev[t], rp[t], Lt, qs, qe);
          dist[ct] = d;
          m.enter<true>(d, ct);
        }
      }
    }
    return m;
  }
  __device__ __forceinline__ void begin_rounds() {}
  __device__ __forceinline__ void retire(double, int i) { dist[i] = INFINITY; }
  __device__ __forceinline__ lmpc_knn_best2 rescan(int lane, double, double, double) {
    lmpc_knn_best2 m;
    m.clear();
    for (int c = lane; c < 3 * n; c += 64) m.enter<true>(dist[c], c);
    return m;
  }
  __device__ __forceinline__ double comp(int j, int k) const { return xl[(size_t)j * 6 + k]; }
  // code = ((row of the point in the concatenated lap store) << 2) | rep
  __device__ __forceinline__ int code(int j, int rep) const { return ((offl + j) << 2) | rep; }
};

__global__ __launch_bounds__(64) void lmpc_ss_query_kernel(int B, int n_laps, int S, int K,
                                                           const int* __restrict__ npts, const int* __restrict__ off,
                                                           const double* __restrict__ x, double Lt,
                                                           const double* __restrict__ query, double* __restrict__ ss_x,
                                                           double* __restrict__ ss_j, int* __restrict__ n_found, double* __restrict__ j0_out,
                                                           int* __restrict__ ss_idx) {
  extern __shared__ __attribute__((aligned(16))) double dist[];
  // XCD-aware query assignment (as in the QP kernel): consecutive workgroups go round-robin to the 8 XCDs, so workgroup
  // w takes query (w mod 8) * ceil(B / 8) + w / 8 and the 8-byte results of neighbouring queries, which share 64-byte
  // lines of the [field][point][batch] arrays, are merged in one XCD's L2 instead of reaching HBM as partial lines
  const int b = (int)(blockIdx.x & 7) * ((B + 7) >> 3) + (int)(blockIdx.x >> 3), lane = threadIdx.x;
  if (b >= B) return;
  lmpc_ss_shared_store st{n_laps, npts, off, x, dist, nullptr, 0, 0};
  lmpc_knn_query(st, B, b, lane, S, K, Lt, query, ss_x, ss_j, n_found, j0_out, ss_idx);
}
