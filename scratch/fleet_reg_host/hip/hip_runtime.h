// Host stand-in for <hip/hip_runtime.h>: just enough to compile csrc/lmpc_fleet_reg_kernel.hip with g++ and run its kernels one
// thread at a time (scratch/fleet_reg_host/check.cpp).  Not a HIP implementation.
#ifndef FLEET_REG_HOST_SHIM_H_
#define FLEET_REG_HOST_SHIM_H_
#include <cmath>
#include <cstddef>
#include <cstdint>
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(...)
struct dim3 {
  unsigned x, y, z;
  dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
struct double2 {
  double x, y;
};
static inline double2 make_double2(double a, double b) { return double2{a, b}; }
typedef void* hipStream_t;
typedef int hipError_t;
extern dim3 blockIdx, threadIdx, blockDim;
static inline void __syncthreads() {}  // the driver runs a workgroup's threads from the last to the first: thread 0 ends it
// A wave of one lane.  (Not `true`, as the track kernel's host build had it: the padding rows of a table are kept out by the VOTE --
// their |z|^2 = 1e30 fails every lane's screen -- while their features are 0, so a lane forced into the hit branch would weigh
// them by |q|^2; on the device no lane can be, the vote being false on every lane.)
#define __any(p) (p)
using std::fmax;  // (sincos: glibc declares it under _GNU_SOURCE, which g++ defines)
#endif
