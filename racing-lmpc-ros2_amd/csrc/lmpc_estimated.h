// lmpc_estimated.h -- the fused estimated period of include/lmpc_hip_estimated.h: the launcher of lmpc_estimated_loop_kernel
// (csrc/lmpc_estimated_loop_kernel.hip), as the host layer calls it (lmpc_loop_advance_estimated_batch in csrc/lmpc_capi.hip).  The
// filter's store and constants are csrc/lmpc_ekf.h's, the spline view csrc/lmpc_track.hip.h's.
#ifndef LMPC_ESTIMATED_H_
#define LMPC_ESTIMATED_H_

#include <hip/hip_runtime.h>

#include "lmpc_device.h"
#include "lmpc_ekf.h"
#include "lmpc_track.hip.h"

struct lmpc_estimated_consts {  // by value in the kernel arguments
  lmpc_vehicle veh;             // the handle's vehicle: plant, filter, reference rollouts, body width
  int N;                        // knots of a plan
  double max_vel_ref_diff;      // the reference sampling's clamp (lmpc_config)
  lmpc_ekf_consts ekf;          // Q and the clip
  lmpc_ekf_obs obs_vel, obs_pose;  // (the host has checked: 1 - 3 rows, within {3, 4, 5} and within {0, 1, 2})
  double dt_vel, dt_pose;       // the two predictions' spans, from the host's clock
};

// Defined in lmpc_estimated_loop_kernel.hip, a translation unit of its own (adding it leaves the device code of the other units as it
// was).  One launch on `stream` for the st.B cars of the filter's store; io's pointers are the caller's, checked by the host layer.
__attribute__((visibility("hidden"))) hipError_t lmpc_estimated_launch(hipStream_t stream, const lmpc_estimated_consts& K, const lmpc_ekf_store& st,
                                                                       const lmpc_track& trk, const lmpc_spline_view& spline,
                                                                       const lmpc_estimated_loop& io);

#endif  // LMPC_ESTIMATED_H_
