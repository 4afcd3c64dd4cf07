// lmpc_fleet_ss.h -- the fleet safe set: one recorder and one ring of laps PER CAR, on the device (csrc/lmpc_fleet_ss_kernel.hip;
// entry points lmpc_fleet_ss_* in csrc/lmpc_capi.hip).
//
// Per car R + 1 lap slots of C samples each (R = lmpc_config.max_lap_stored, C = max_pts_per_lap): R closed laps -- the
// boost::circular_buffer of SafeSetManager (safe_set.cpp:139-151) -- and the open lap SafeSetRecorder is filling (:278-322).  The
// open lap is recorded IN PLACE in slot `head`; closing it moves nothing: head steps on to the next slot, which is either unused or
// holds the oldest lap (then evicted).  The ring is the `cnt` slots behind head, newest at head - 1.
//
// A sample is 80 bytes in three planes, so that the query streams 16 of them:
//   key [car][slot][C]     (s, e_y)                         16 B   what the k-NN scan reads
//   xr  [car][slot][C][4]  (e_psi, vx, vy, omega)           32 B   gathered for the <= S winners only
//   aux [car][slot][C][4]  (u_lon, steer, curvature, t)     32 B   read by lmpc_fleet_ss_get_laps (lap files) and by the per-car
//                                                                   regression's pack kernel (lmpc_fleet_reg_kernel.hip)
#ifndef LMPC_FLEET_SS_H_
#define LMPC_FLEET_SS_H_

#include <hip/hip_runtime.h>

#define LMPC_FLEET_DUR 8  // closed-lap durations kept per car

struct lmpc_fleet_store {
  int B = 0, R = 0, C = 0;  // cars, laps in a car's ring, samples in a lap slot
  double2* key = nullptr;
  double* xr = nullptr;
  double* aux = nullptr;
  // per-car recorder and ring state; all zero = a car that has seen nothing
  int* npts = nullptr;       // [B][R + 1] samples of the closed lap in a slot
  int* head = nullptr;       // [B] slot of the open lap
  int* cnt = nullptr;        // [B] closed laps in the ring
  int* open_n = nullptr;     // [B] samples stored in the open lap
  int* flags = nullptr;      // [B] bit 0 last_x_valid, bit 1 initialized (safe_set.cpp:278-300), bit 2 the open lap overflowed
  int* lap_count = nullptr;  // [B] SafeSetRecorder::lap_count_
  int* n_dropped = nullptr;  // [B] closed laps refused for their length
  int* dur_n = nullptr;      // [B] durations pushed so far
  double* s_prev = nullptr;  // [B] abscissa of the previous sample (last_x_[0])
  double* dur = nullptr;     // [B][LMPC_FLEET_DUR] ring of lap durations
};

#define LMPC_FLEET_FLAG_VALID 1
#define LMPC_FLEET_FLAG_INIT 2
#define LMPC_FLEET_FLAG_OVERFLOW 4

__global__ void lmpc_fleet_ss_record_kernel(lmpc_fleet_store, const double*, const double*, const double*, double, double, const int*);
__global__ void lmpc_fleet_ss_query_kernel(lmpc_fleet_store, int, int, double, const double*, double*, double*, int*);
__global__ void lmpc_fleet_ss_load_kernel(lmpc_fleet_store, int, int, const int*, const int*, const double*, const double*, const double*,
                                          const double*);
__global__ void lmpc_fleet_ss_stats_kernel(lmpc_fleet_store, int*, int*, int*, double*);

#endif  // LMPC_FLEET_SS_H_
