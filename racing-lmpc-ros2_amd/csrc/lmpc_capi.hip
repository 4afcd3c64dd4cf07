// lmpc_capi.hip -- host side of the C ABI declared in include/lmpc_hip.h (gfx950 / ROCm).
//
// The handle owns: the digested parameter block (the reference builds its parametric problem
// once in RacingMPC::RacingMPC, racing_mpc.cpp:31-202), one HIP stream, the linearisation
// workspace and the device copy of the safe set.  Nothing here computes on the hot path; the
// product fails loudly (negative return code + message) rather than falling back to a CPU path.
//
// Compiled as the last include of lmpc_lib.hip, behind every kernel's definition.  Layout: the buffer owners and the handle;
// one anonymous namespace with the helpers, each before its users (which kernel runs: `kernel_table` / `choose_kernel`; how it
// is launched: `launch_params` / `launch_solve`; what a solve is asked: `solve_args`); the exported functions.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "lmpc_device.h"
#include "lmpc_ekf.h"
#include "lmpc_lqr.h"
#include "lmpc_vanilla.h"
#include "lmpc_fleet_reg.h"
#include "lmpc_reg_rows.h"
#include "lmpc_fleet_ss.h"
#include "lmpc_fleet_loop.h"
#include "lmpc_cars.h"
#include "lmpc_dtrack.h"
#include "lmpc_dtrack_model.h"
#include "lmpc_cars_model.h"
#include "lmpc_estimated.h"

namespace {
// Move-only owner of one device (PINNED: pinned host) allocation: freed by the destructor, and by alloc() before it allocates anew.
template <typename T, bool PINNED>
class hip_buf {
  T* p = nullptr;

 public:
  hip_buf() = default;
  hip_buf(hip_buf&& o) noexcept : p(o.p) { o.p = nullptr; }
  hip_buf& operator=(hip_buf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      o.p = nullptr;
    }
    return *this;
  }
  ~hip_buf() { release(); }
  T* get() const { return p; }
  void release() {
    if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
    p = nullptr;
  }
  hipError_t alloc(size_t n) {  // n elements; on failure the owner is empty
    release();
    const hipError_t e = PINNED ? hipHostMalloc(&p, n * sizeof(T)) : hipMalloc(&p, n * sizeof(T));
    if (e != hipSuccess) p = nullptr;
    return e;
  }
};
template <typename T>
using dev_buf = hip_buf<T, false>;
template <typename T>
using pinned_buf = hip_buf<T, true>;
}  // namespace

struct __attribute__((visibility("hidden"))) lmpc_handle {  // (its members are no part of the library's ABI)
  lmpc_params P;
  lmpc_config cfg;
  int device = 0;
  hipStream_t stream = nullptr;  // nullptr = the device's default (null) stream
  bool out_aos = false;  // lmpc_set_output_layout: applies to lmpc_solve_batch / lmpc_solve_batch_mixed as the CALLER invokes them; every
                         // solve the library launches for itself (the SQP's QPs, the single-problem host path) writes the default layout
  const int* order = nullptr;  // lmpc_set_launch_order: device [order_n], applied to solves of that batch size only
  int order_n = 0;
  int warm_rounds = 0;    // lmpc_set_warm_rounds (0: by batch size, see launch_params)
  int warm_resident = 0;  // problems the device holds at once in the warm kernel (CUs x workgroups per CU); 0: no warm kernel for this handle
  dev_buf<double> ws;       // [ws_cap][N-1][LMPC_LIN_RECORD]
  dev_buf<int> unverified;  // [ws_cap + 1]: the problems a mixed first pass could not verify, and their number
  dev_buf<int> warm_flag;   // [ws_cap]: 1 where the last warm solve's attempt was accepted (written by the warm kernels)
  int warm_flag_n = 0;      // the batch of the solve that wrote it (0: no warm solve since)
  dev_buf<char> save;       // [save_cap] bytes = problems x element size, times 10 N - 4: the polish's save area (grown by
  size_t save_cap = 0;      // reserve_save; P.save follows it)
  size_t ws_cap = 0;
  dev_buf<float> ws_f32;  // the same for the single-precision solve
  size_t ws_f32_cap = 0;
  // safe set (device): laps newest-first offsets
  int ss_laps = 0;
  int ss_total = 0;
  dev_buf<int> ss_npts, ss_off;
  dev_buf<double> ss_x;  // [total][6]
  double ss_L = 0.0;
  int ss_nmax = 0;
  unsigned ss_gen = 0;      // bumped by every lmpc_set_safe_set: the store the codes of lmpc_ss_query_idx_batch point into
  unsigned ss_idx_gen = 0;  // the generation the last lmpc_ss_query_idx_batch ran against (0: none yet)
  int last_precision = LMPC_PRECISION_F64;  // what the last batched solve ran in (lmpc_last_solve_precision)
  int waves = 0;  // lmpc_set_waves_per_problem: 0 the library's choice, 1 / 2 forced (2: fp64 tracking problem, N >= 24, cold solves)
  // regression store (device): lap samples, one-step residuals of the nominal model, end-of-lap flags
  bool reg_on = false;
  int reg_total = 0;
  dev_buf<int> reg_end;
  dev_buf<double> reg_x;    // [total][6]
  dev_buf<double> reg_u;    // [total][2]
  dev_buf<double> reg_y;    // [total][6]
  dev_buf<double> reg_tab;  // [reg_npad][NF + NOUT]: features and regressed residuals of the samples that have a successor,
                            // and behind them [reg_npad]: the features' squared norms
  int reg_npad = 0;         // their number, padded to a multiple of four with unreachable rows
  bool reg_exact = false;   // features large against the bandwidth: the kernel recomputes each weight from sum (z - q)^2
  lmpc_regression_spec reg_spec{};
  // one feature list per regressed row (lmpc_set_regression_laps_rows; csrc/lmpc_reg_rows.h): reg_on with reg_rows set -- the same
  // store, reg_tab in the per-row layout [reg_npad][3 mf + 3], reg_rspec in place of reg_spec
  bool reg_rows = false;
  lmpc_reg_rows_dev reg_rspec{};
  // fleet safe set (lmpc_fleet_ss_create): one recorder and one ring of laps per car, csrc/lmpc_fleet_ss.h
  lmpc_fleet_store fleet{};  // raw copies of the five owners below, as the kernels take them
  dev_buf<double2> fleet_key;
  dev_buf<double> fleet_xr, fleet_aux;
  dev_buf<int> fleet_meta;      // the store's per-car int arrays, one allocation (zeroed by lmpc_fleet_ss_reset)
  dev_buf<double> fleet_metad;  // and its per-car double arrays
  size_t fleet_meta_n = 0, fleet_metad_n = 0;
  int64_t fleet_bytes = 0;
  double fleet_L = 0.0;  // total_length of the last record / load call: what the query unrolls the laps by
  // per-car regression on the fleet store (lmpc_fleet_ss_set_regression): csrc/lmpc_fleet_reg.h
  bool freg_on = false;
  lmpc_regression_spec freg_spec{};
  bool freg_rows = false;  // lmpc_fleet_ss_set_regression_rows: freg_on with freg_rspec in place of freg_spec, the table in the per-row layout
  lmpc_reg_rows_dev freg_rspec{};
  lmpc_fleet_reg_table freg{};  // raw copies of the two owners below, as the kernels take them
  dev_buf<double> freg_tab;     // [fleet.B][freg.cap][NF + NOUT + 1]
  dev_buf<int> freg_meta;       // nrow [fleet.B] | stamp [fleet.B]
  int64_t freg_bytes = 0;
  // car table (lmpc_cars_set_vehicles): one plant vehicle per car, csrc/lmpc_cars.h
  dev_buf<double> cars_tab;  // [lmpc_cars_fields][cars_B] doubles | integrator int32 [cars_B]
  int cars_B = 0;            // 0: no table
  bool cars_model = false;   // lmpc_cars_set_controller_model: the batched solves linearise problem b on vehicle b of the car table
  // double-track table (lmpc_dtrack_set_vehicles): one four-wheel plant vehicle per car, csrc/lmpc_dtrack.h
  dev_buf<double> dtrack_tab;  // [lmpc_dtrack_fields][dtrack_B] doubles | integrator int32 [dtrack_B]
  int dtrack_B = 0;            // 0: no table
  bool dtrack_model = false;   // lmpc_dtrack_set_controller_model: solve_batch linearises problem b on vehicle b of the table
  // batched extended Kalman filter (lmpc_ekf_create): one filter per car, csrc/lmpc_ekf.h
  lmpc_ekf_store ekf{};  // raw copies of the two owners below, as the kernels take them
  dev_buf<double> ekf_xup;  // x [6][B] | u [2][B] | P [36][B]
  dev_buf<double> ekf_K;    // [6][nzsum][B], allocated anew by every registration
  std::vector<lmpc_ekf_obs> ekf_obs;
  lmpc_ekf_config ekf_cfg{};
  bool ekf_initialized = false;  // initialized_ upstream: registration is closed, updates are open
  int64_t ekf_ns = 0;            // nanosec_: the time of the last update
  // batched time-varying LQR (lmpc_lqr_create): one controller per car, csrc/lmpc_lqr.h
  lmpc_lqr_store lqr{};     // raw copies of the owner below, as the kernels take them
  dev_buf<double> lqr_ws;   // cfg [76] | AB [N-1][8][max_batch][6] | K [N-1][2][max_batch][6]
  // batched vanilla controller (lmpc_vanilla_create): one pure-pursuit + PID controller per car, csrc/lmpc_vanilla.h
  lmpc_vanilla_store vanilla{};  // the config and a raw copy of the owner below, as the kernels take them
  dev_buf<double> vanilla_pid;   // [3][batch]: integral | error | last_error
  // staging for the single-problem host entry points (lmpc_solve_host, lmpc_ss_query_host): device buffers and PINNED
  // host mirrors, all sized and allocated by lmpc_create -- the per-step path of one controller allocates nothing
  dev_buf<double> stage_dev;
  pinned_buf<double> stage_host;
  size_t stage_doubles = 0;
  dev_buf<int> stage_int;
  pinned_buf<int> stage_int_host;
  dev_buf<double> ssq_dev;  // query [2] | ss_x [6][S] | ss_j [S] | j0
  pinned_buf<double> ssq_host;
  dev_buf<int> ssq_int;
  pinned_buf<int> ssq_int_host;
  // work area of lmpc_solve_full_dynamics_batch (grown by its first call for a batch size, like the workspace)
  dev_buf<double> sqp_ws;
  dev_buf<int> sqp_int;
  size_t sqp_cap = 0;
  pinned_buf<int> sqp_count_host;
  // timing
  bool timing = false;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  std::string err;

  ~lmpc_handle() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// A spline track (lmpc_spline_track_create): the device copy of RacingTrajectory's piecewise cubics and waypoints; `view` is what the
// kernels of lmpc_track_kernel.hip take.
struct __attribute__((visibility("hidden"))) lmpc_spline_track {
  lmpc_spline_view view{};
  int device = 0;
  dev_buf<double> breaks, coef, wp_xy, wp_s;
};

namespace {

int fail(lmpc_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  return code;
}

// `who`: what the message names -- the failing expression (HIP_TRY), or the entry point where it reports under its own name.  The
// runtime's sticky error is cleared: a refused allocation would otherwise surface at the next launch's hipGetLastError.
#define HIP_TRY_AS(h, who, expr)                                                                 \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess) {                                                                      \
      (void)hipGetLastError();                                                                   \
      return fail(h, LMPC_ERR_RUNTIME, std::string(who) + ": " + hipGetErrorString(e_));         \
    }                                                                                            \
  } while (0)
#define HIP_TRY(h, expr) HIP_TRY_AS(h, #expr, expr)

// Grow-on-demand of what `cap` counts: the stream is drained before anything it may still read is released, `allocate` (which
// returns a status) replaces the buffers, and the capacity is raised only after everything succeeded -- a failure leaves it zero,
// so the next call reserves again instead of using what is not there.
template <typename F>
int grow(lmpc_handle* h, size_t& cap, size_t want, F&& allocate) {
  if (want <= cap) return LMPC_OK;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  cap = 0;
  const int rc = allocate();
  if (rc == LMPC_OK) cap = want;
  return rc;
}

// ---- which kernel runs ----
// One row per (KQ, KS) class: KQ = slots per lane, lmpc_slot_class(N) (2 / 4 / 7 / 11 / 14 for N <= 11 / 23 / 40 / 64 / 81);
// KS = 0 the tracking problem, 2 up to 128 safe-set points, 3 up to 192.  The columns name exactly the instantiations of
// lmpc_solve_kernel.hip's list (naming another one here would instantiate it); null: not built for that class.
struct kernel_row {
  int kq, ks;
  const void *f64, *w2, *mixed, *f32, *second, *warm;
};
#define F64(KQ, KS) reinterpret_cast<const void*>(&lmpc_solve_kernel<double, KQ, KS, double>)
#define W2(KQ) reinterpret_cast<const void*>(&lmpc_solve_kernel_w2<KQ>)  // two wavefronts per problem (csrc/lmpc_solve_w2.hip.h)
#define MIX(KQ, KS) reinterpret_cast<const void*>(&lmpc_solve_kernel<float, KQ, KS, double>)  // fp32 iteration between fp64 arrays
#define F32(KQ) reinterpret_cast<const void*>(&lmpc_solve_kernel<float, KQ, 0, float>)        // fp32 arrays and iteration
#define SEC(KQ, KS) reinterpret_cast<const void*>(&lmpc_cleanup_kernel<double, KQ, KS, double>)  // the fp64 second pass of a mixed solve
#define WARM(KQ, KS) reinterpret_cast<const void*>(&lmpc_solve_warm_kernel<KQ, KS>)
// N <= 11 has a kernel of its own for the fp64 tracking problem, cold and warm; everything else runs it on the KQ = 4 kernels.
// The mixed learning problem: N <= 23 (BASELINE configs[4]).  N = 40 stays fp64: built for the experiment (round 3, two-pass, the
// fp32 kernel at one wave per SIMD) it ran 0.80 M solves/s against 0.70 M in fp64 with 13 % of the batch going to the
// second pass, and one problem of 4096 passed its single-precision KKT test 3.6e-3 away from the fp64 answer -- outside
// the 1e-3 this entry states, for a 1.14x gain
// (the N = 40 / 60 instantiations of that experiment, -DLMPC_MIXED_LONG_LEARNING until round 5: scratch/r5/experiment_switches.patch)
// The learning problem's warm start: up to N = 60 (KQ = 11).
const kernel_row kernel_table[] = {
//   KQ  KS fp64 cold   2 waves  mixed       fp32     2nd pass    warm
    {2,  0, F64(2, 0),  nullptr, MIX(4, 0),  F32(4),  SEC(4, 0),  WARM(2, 0)},
    {4,  0, F64(4, 0),  nullptr, MIX(4, 0),  F32(4),  SEC(4, 0),  WARM(4, 0)},
    {7,  0, F64(7, 0),  W2(7),   MIX(7, 0),  F32(7),  SEC(7, 0),  WARM(7, 0)},
    {11, 0, F64(11, 0), W2(11),  MIX(11, 0), F32(11), SEC(11, 0), WARM(11, 0)},
    {14, 0, F64(14, 0), W2(14),  MIX(14, 0), F32(14), SEC(14, 0), WARM(14, 0)},
    {2,  2, F64(4, 2),  nullptr, MIX(4, 2),  nullptr, SEC(4, 2),  WARM(4, 2)},
    {4,  2, F64(4, 2),  nullptr, MIX(4, 2),  nullptr, SEC(4, 2),  WARM(4, 2)},
    {7,  2, F64(7, 2),  nullptr, nullptr,    nullptr, nullptr,    WARM(7, 2)},
    {11, 2, F64(11, 2), nullptr, nullptr,    nullptr, nullptr,    WARM(11, 2)},
    {14, 2, F64(14, 2), nullptr, nullptr,    nullptr, nullptr,    nullptr},
    {2,  3, F64(4, 3),  nullptr, MIX(4, 3),  nullptr, SEC(4, 3),  WARM(4, 3)},
    {4,  3, F64(4, 3),  nullptr, MIX(4, 3),  nullptr, SEC(4, 3),  WARM(4, 3)},
    {7,  3, F64(7, 3),  nullptr, nullptr,    nullptr, nullptr,    WARM(7, 3)},
    {11, 3, F64(11, 3), nullptr, nullptr,    nullptr, nullptr,    WARM(11, 3)},
    {14, 3, F64(14, 3), nullptr, nullptr,    nullptr, nullptr,    nullptr},
};
#undef F64
#undef W2
#undef MIX
#undef F32
#undef SEC
#undef WARM

int ks_for(int S) { return S <= 0 ? 0 : (S <= 128 ? 2 : (S <= 192 ? 3 : -1)); }

// which cold fp64 tracking solves take the two-wave kernels: forced by lmpc_set_waves_per_problem, else by measurement (LMPC_W2_AUTO_KQ:
// the smallest one-wave slot count from which two waves are the default)
#define LMPC_W2_AUTO_KQ 11  // N >= 41 (with the fused factorisation in both): N = 80 9.70 -> 8.06 ms per 4096, N = 65 6.59 -> 5.32, N = 41 .. 64 -1 .. 4 %; N <= 40 +5 %: one wave (profiles/r06_fuse_ab.txt)

// what is asked of a handle: the cold solve of an entry point (SOLVE_F64: as lmpc_solve_batch launches it, one or two waves;
// SOLVE_F64_ONE_WAVE: whatever the wave setting), the fp64 second pass of a mixed solve, the warm start
enum solve_kind { SOLVE_F64, SOLVE_F64_ONE_WAVE, SOLVE_MIXED, SOLVE_F32, SOLVE_SECOND_PASS, SOLVE_WARM };

struct launch_choice {
  const void* fn = nullptr;  // null: no kernel is built for this handle's (N, num_ss_pts) and this kind
  int threads = 64;          // per problem
  size_t lds = 0;            // bytes per problem
};

// THE dispatch decision: what a solve of this kind on this handle launches.  The solve path and the lmpc_query_* functions all ask here.
launch_choice choose_kernel(const lmpc_handle* h, solve_kind kind) {
  const int kq = lmpc_slot_class(h->P.N), ks = ks_for(h->P.S);
  launch_choice c;
  c.lds = lmpc_lds_bytes(h->P.N, h->P.learning, h->P.S, (kind == SOLVE_MIXED || kind == SOLVE_F32) ? 4 : 8);
  for (const kernel_row& r : kernel_table) {
    if (r.kq != kq || r.ks != ks) continue;
    const bool two_waves = kind == SOLVE_F64 && r.w2 && (h->waves == 2 || (h->waves == 0 && kq >= LMPC_W2_AUTO_KQ));
    c.threads = two_waves ? 128 : 64;
    c.fn = two_waves                    ? r.w2
           : kind == SOLVE_MIXED        ? r.mixed
           : kind == SOLVE_F32          ? r.f32
           : kind == SOLVE_SECOND_PASS  ? r.second
           : kind == SOLVE_WARM         ? r.warm
                                        : r.f64;
  }
  return c;
}

// how many problems of that launch a CU holds at once
int residency(lmpc_handle* h, const launch_choice& k, int* per_cu) {
  HIP_TRY(h, hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds));
  HIP_TRY(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, k.fn, k.threads, k.lds));
  return LMPC_OK;
}

// ---- what a solve is asked ----
// The request of one batched solve, as the exported functions fill it: the arrays every entry point requires, in the order of the
// C ABI, then what only some of them have (null / zero: not asked).  `io` is the type of the caller's arrays.
template <typename io = double>
struct solve_args {
  int B;
  const io *x_ic, *u_ic, *X_ref, *U_ref, *T_ref, *bl, *br, *curv, *vref;
  io *X, *U, *dU;
  int *status, *iters;
  io* kkt = nullptr;
  const io *ss_x = nullptr, *ss_j = nullptr;  // learning: the safe-set points as arrays ...
  const int* ss_idx = nullptr;                // ... or by reference (lmpc_solve_batch_ss_idx)
  io* lam = nullptr;                          // learning: convex_combi_optm
  const io *warm_X = nullptr, *warm_U = nullptr;  // lmpc_solve_batch_warm: the plan of the active-set attempt (null: cold)
  const io* warm_lam = nullptr;                   // ... and, learning, the plan's simplex weights [S][B]
  bool mixed = false;  // fp32 iteration between these fp64 arrays
  bool aos = false;    // results [batch][knot][component]
  // the single-problem host entries (solve_host): max_sqp > 0 the full-dynamics solve and its three reports
  int max_sqp = 0;
  double step_tol = 0.0;
  int* sqp_iters = nullptr;
  double *sqp_move = nullptr, *defect = nullptr;
};

// ---- how it is launched ----
// The per-launch copy of the parameter block.  Which field each kind of launch gets:
//   launch_order     every solve of exactly the registered batch size; never the second pass (it walks its own list)
//   (fp32 arrays get nothing else: the tracking problem, cold, in the default layout whatever lmpc_set_output_layout says)
//   out_aos, the safe set by reference, the warm plan   as the request says
//   flag_unverified  the fp32 iteration of a mixed solve whose polish runs (it marks what it could not verify)
//   warm_rounds, warm_flag   the warm launch only
template <typename io>
lmpc_params launch_params(const lmpc_handle* h, const solve_args<io>& a, solve_kind kind) {
  lmpc_params P = h->P;
  // the registered order applies to solves of exactly its own batch size; every other launch through this handle (the
  // single-problem host path, the SQP's QPs on another batch, ...) keeps the default mapping
  P.launch_order = (kind != SOLVE_SECOND_PASS && h->order && a.B == h->order_n) ? h->order : nullptr;
  if constexpr (std::is_same<io, double>::value) {  // (the fp32 entry stops here)
    P.out_aos = a.aos ? 1 : 0;
    P.flag_unverified = (kind == SOLVE_MIXED && h->P.polish >= 0) ? 1 : 0;
    // the safe set by reference: the codes of lmpc_ss_query_idx_batch and the handle's lap store they point into
    P.ss_idx = a.ss_idx;
    P.ss_store = h->ss_x.get();
    P.ss_npts = h->ss_npts.get();
    P.ss_off = h->ss_off.get();
    P.ss_laps = h->ss_laps;
    P.ss_rows = h->ss_total;
    P.ss_L = h->ss_L;
    P.warm_X = a.warm_X;
    P.warm_U = a.warm_U;
    P.warm_lam = a.warm_lam;
    P.warm_flag = nullptr;
    if (kind == SOLVE_WARM) {
      // Repair rounds before the cold start takes over.  A refused attempt is the longest job of its batch (its rounds + a cold solve)
      // and an accepted one the shortest: while the batch fits the device a few times over, its duration is that of the longest jobs
      // and a refusal should come early (2 rounds: 95 % accepted at N = 20, 73 % at N = 60); once the batch is many times what the
      // device holds, throughput counts and every cold solve saved pays (4 rounds: 99 % / 89 %).  Measured in the closed loop
      // (profiles/r05_closed_loop_warm_rounds.txt): N = 20, 4096 cars (2 x resident) 5.50 / 5.36 / 5.17 M car-steps/s at 2 / 3 / 4
      // rounds, 16384 cars (8 x) 10.43 / 10.64 / 10.54; N = 60, 4096 cars (4 x) 1.00 / 1.02 / 1.05.
      P.warm_rounds = h->warm_rounds > 0 ? h->warm_rounds : ((h->warm_resident > 0 && a.B >= 4 * h->warm_resident) ? 4 : 2);
      P.warm_flag = h->warm_flag.get();  // (reserved with the workspace: at least a.B entries)
    }
  }
  return P;
}

// THE launch of a solve kernel: LDS attribute, per-launch parameters, argument list, grid.  `ws`: the linearisation workspace in the
// arrays' type.  The kernels' argument lists differ in two places: the second pass takes its list and count in front, and the
// two-wave kernels (tracking only) have no safe-set and weight arguments.
template <typename io>
int launch_solve(lmpc_handle* h, solve_kind kind, launch_choice k, const solve_args<io>& a, const io* ws) {
  const bool two_waves = k.threads == 128, second = kind == SOLVE_SECOND_PASS;
#ifdef LMPC_DEBUG_HOOKS  // (measurement builds only, `make debug`)
  // LMPC_LDS_PAD (bytes): over-allocate LDS per problem to cap the problems resident on a CU (the one-wave cold solves)
  static const int lds_pad = [] { const char* e = getenv("LMPC_LDS_PAD"); return e ? atoi(e) : 0; }();
  if ((kind == SOLVE_F64 || kind == SOLVE_MIXED) && !two_waves) k.lds += lds_pad;
  static const bool wide = getenv("LMPC_DEBUG_CLEANUP_WIDE") != nullptr;  // the second pass on one workgroup per problem
#else
  const bool wide = false;
#endif
  HIP_TRY(h, hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds));
  lmpc_params P = launch_params(h, a, kind);
  if (kind == SOLVE_WARM) h->warm_flag_n = a.B;
  int B = a.B;
  const int* list = h->unverified.get();
  const int* count = list + a.B;
  void* args[20];
  int n = 0;
  auto push = [&](const void* p) { args[n++] = const_cast<void*>(p); };
  push(&P), push(&B);
  if (second) push(&list), push(&count);
  push(&ws), push(&a.x_ic), push(&a.u_ic), push(&a.T_ref), push(&a.bl), push(&a.br), push(&a.vref);
  if (!two_waves) push(&a.ss_x), push(&a.ss_j), push(&a.lam);
  push(&a.X), push(&a.U), push(&a.dU), push(&a.status), push(&a.iters), push(&a.kkt);
  // one workgroup per problem, rounded up to the 8 XCDs (see the kernel: XCD-aware mapping); the second pass: a percent of a
  // batch is marked, 1024 workgroups take them in one or two turns
  const int grid = second ? ((a.B < 1024 || wide) ? a.B : 1024) : 8 * ((a.B + 7) / 8);
  HIP_TRY(h, hipLaunchKernel(k.fn, dim3(grid), dim3(k.threads), args, k.lds, h->stream));
  return LMPC_OK;
}

// the linearisation onto a workspace; real_bytes: what the QP kernel behind it iterates in
template <typename io>
int launch_linearize(lmpc_handle* h, int real_bytes, int batch, const io* X_ref, const io* U_ref, const io* T_ref, const io* curv, io* ws) {
  const dim3 grid((batch + 255) / 256, h->P.N - 1);
  // the 256-register build of the linearisation where a wave of it can sit next to a resident wave of the QP kernel that follows
  // (two waves per SIMD: the short-horizon tracking kernels), so that the next batch's linearisation fills this batch's residency tail
  if (!h->P.learning && lmpc_waves_per_simd(real_bytes, lmpc_slot_class(h->P.N), 0) >= 2)
    hipLaunchKernelGGL((lmpc_linearize_kernel<true, io, 2>), grid, dim3(256), 0, h->stream, h->P, batch, X_ref, U_ref, T_ref, curv, ws,
                       (io*)nullptr, (io*)nullptr);
  else
    hipLaunchKernelGGL((lmpc_linearize_kernel<true, io, 1>), grid, dim3(256), 0, h->stream, h->P, batch, X_ref, U_ref, T_ref, curv, ws,
                       (io*)nullptr, (io*)nullptr);
  HIP_TRY(h, hipGetLastError());
  return LMPC_OK;
}

// one lane per (problem, stage); WS: the handle's workspace, otherwise the caller's A/B/g arrays
template <bool WS>
int launch_regress(lmpc_handle* h, int batch, const double* X_ref, const double* U_ref, double* A, double* Bm, double* g) {
  const int nf = h->reg_spec.n_in_state + h->reg_spec.n_in_ctrl;
  const long long queries = (long long)batch * (h->P.N - 1);
  const dim3 grid((unsigned)((queries + 63) / 64)), block(64);
  const double* tab = h->reg_tab.get();
  if (h->reg_rows) {  // one feature list per row: one pass of lmpc_regress_rows_kernel for all rows
    if (h->reg_rspec.mf == 4)
      hipLaunchKernelGGL((lmpc_regress_rows_kernel<4, WS>), grid, block, 0, h->stream, h->P.N, batch, h->reg_rspec, h->reg_npad, tab, X_ref, U_ref, A,
                         Bm, g);
    else
      hipLaunchKernelGGL((lmpc_regress_rows_kernel<5, WS>), grid, block, 0, h->stream, h->P.N, batch, h->reg_rspec, h->reg_npad, tab, X_ref, U_ref, A,
                         Bm, g);
    HIP_TRY(h, hipGetLastError());
    return LMPC_OK;
  }
  const double* zz = tab + (size_t)h->reg_npad * (size_t)(nf + h->reg_spec.n_out);
  const bool five = nf == 5 && h->reg_spec.n_out == 3;
  const void* fn = h->reg_exact ? (five ? (const void*)lmpc_regress_kernel<5, 3, WS, true> : (const void*)lmpc_regress_kernel<8, 6, WS, true>)
                                : (five ? (const void*)lmpc_regress_kernel<5, 3, WS, false> : (const void*)lmpc_regress_kernel<8, 6, WS, false>);
  int N = h->P.N, npad = h->reg_npad;
  lmpc_regression_spec spec = h->reg_spec;
  void* args[] = {(void*)&N, (void*)&batch, (void*)&spec, (void*)&npad, (void*)&tab, (void*)&zz, (void*)&X_ref, (void*)&U_ref,
                  (void*)&A, (void*)&Bm, (void*)&g};
  HIP_TRY(h, hipLaunchKernel(fn, grid, block, args, 0, h->stream));
  HIP_TRY(h, hipGetLastError());
  return LMPC_OK;
}

// the per-car regression (lmpc_fleet_ss_set_regression is in effect): pack what changed, then one wavefront per (car, 64 stages)
int launch_fleet_regress(lmpc_handle* h, bool ws, const double* X_ref, const double* U_ref, double* A, double* Bm, double* g) {
  if (h->freg_rows)
    HIP_TRY(h, lmpc_fleet_reg_rows_launch(h->stream, h->fleet, h->P.veh, h->freg_rspec, h->freg, h->P.N, ws, X_ref, U_ref, A, Bm, g));
  else
    HIP_TRY(h, lmpc_fleet_reg_launch(h->stream, h->fleet, h->P.veh, h->freg_spec, h->freg, h->P.N, ws, X_ref, U_ref, A, Bm, g));
  return LMPC_OK;
}

// what lmpc_fleet_ss_set_regression asks of a solve: the store's own batch (query (b, i) runs against car b's laps)
int fleet_reg_batch_check(lmpc_handle* h, int batch, const char* who) {
  if (!h->freg_on || batch == h->fleet.B) return LMPC_OK;
  return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": the per-car regression is on (lmpc_fleet_ss_set_regression) and batch " +
                                        std::to_string(batch) + " is not the fleet store's " + std::to_string(h->fleet.B));
}

// every stamp stale, on the stream: the next regression packs every car again
int fleet_reg_invalidate(lmpc_handle* h) {
  if (h->freg_on) HIP_TRY(h, hipMemsetAsync(h->freg.stamp, 0xff, (size_t)h->fleet.B * sizeof(int), h->stream));
  return LMPC_OK;
}

// off, and its table freed (the stream is drained first: a launch may still read it)
void fleet_reg_off(lmpc_handle* h) {
  if (h->freg_tab.get() || h->freg_meta.get()) (void)hipStreamSynchronize(h->stream);
  h->freg_tab.release();
  h->freg_meta.release();
  h->freg = lmpc_fleet_reg_table{};
  h->freg_on = false;
  h->freg_rows = false;
  h->freg_bytes = 0;
}

// the shared regression off, in either form, and its store freed (the caller has drained the stream: a launch may still read it)
void reg_off(lmpc_handle* h) {
  h->reg_end.release();
  h->reg_x.release();
  h->reg_u.release();
  h->reg_y.release();
  h->reg_tab.release();
  h->reg_npad = 0;
  h->reg_exact = false;
  h->reg_on = false;
  h->reg_rows = false;
  h->reg_total = 0;
}

// The laps of the shared regression, either form, onto the device: end-of-lap flags, states, inputs and the nominal model's one-step
// residuals (reg_end, reg_x, reg_u, reg_y); `valid` = the samples that have a successor, in order.  The kernel has run when it returns.
int reg_upload_laps(lmpc_handle* h, const char* who, int32_t n_laps, const int32_t* n_pts, const double* x, const double* u, const double* k,
                    const double* t, bool as_written, std::vector<int>& valid) {
  size_t total = 0;
  std::vector<int> end;
  for (int l = 0; l < n_laps; ++l) {
    if (n_pts[l] < 2) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": a lap needs two samples");
    total += (size_t)n_pts[l];
    end.resize(total, 0);
    end[total - 1] = 1;
  }
  dev_buf<double> dk, dt;  // upload-time temporaries: freed on every way out of this function
  HIP_TRY(h, h->reg_end.alloc(total));
  HIP_TRY(h, h->reg_x.alloc(total * 6));
  HIP_TRY(h, h->reg_u.alloc(total * 2));
  HIP_TRY(h, h->reg_y.alloc(total * 6));
  HIP_TRY(h, dk.alloc(total));
  HIP_TRY(h, dt.alloc(total));
  HIP_TRY(h, hipMemcpy(h->reg_end.get(), end.data(), total * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(h, hipMemcpy(h->reg_x.get(), x, total * 6 * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(h, hipMemcpy(h->reg_u.get(), u, total * 2 * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(h, hipMemcpy(dk.get(), k, total * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(h, hipMemcpy(dt.get(), t, total * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(lmpc_reg_residual_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, h->P.veh,
                     (int)total, as_written ? 1 : 0, h->reg_end.get(), h->reg_x.get(), h->reg_u.get(), dk.get(), dt.get(),
                     h->reg_y.get());
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // dk and dt are read by it
  valid.clear();
  valid.reserve(total);
  for (size_t j = 0; j < total; ++j)
    if (!end[j]) valid.push_back((int)j);
  h->reg_total = (int)total;
  return LMPC_OK;
}

// The per-car tables of either form, `stride` doubles per sample: refuses a store too large for a car's table, allocates when the size
// differs from what is there (the only case that drains the stream), and leaves every car to be packed again.
int fleet_reg_table_setup(lmpc_handle* h, const char* who, size_t stride) {
  if ((long long)h->fleet.R * (h->fleet.C - 1) > (1ll << 30))
    return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": max_lap_stored x max_pts_per_lap is too large for a car's table");
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t Bz = (size_t)h->fleet.B;
  const int cap = lmpc_fleet_reg_cap(h->fleet.R, h->fleet.C);
  const size_t tab_n = Bz * (size_t)cap * stride;
  if (!h->freg_on || cap != h->freg.cap || tab_n * sizeof(double) + 2 * Bz * sizeof(int) != (size_t)h->freg_bytes) {
    fleet_reg_off(h);
    // into local owners: a refused allocation leaves the regression off, and nothing behind
    dev_buf<double> tab;
    dev_buf<int> meta;
    HIP_TRY_AS(h, who, tab.alloc(tab_n ? tab_n : 1));
    HIP_TRY_AS(h, who, meta.alloc(2 * Bz));
    h->freg_tab = std::move(tab);
    h->freg_meta = std::move(meta);
    h->freg.cap = cap;
    h->freg.tab = h->freg_tab.get();
    h->freg.nrow = h->freg_meta.get();
    h->freg.stamp = h->freg_meta.get() + Bz;
    h->freg_bytes = (int64_t)(tab_n * sizeof(double) + 2 * Bz * sizeof(int));
  }
  // behind every launch that still reads the old spec's table: no row count, and every stamp stale (a new spec or sign convention
  // changes every row)
  HIP_TRY(h, hipMemsetAsync(h->freg.nrow, 0, Bz * sizeof(int), h->stream));
  HIP_TRY(h, hipMemsetAsync(h->freg.stamp, 0xff, Bz * sizeof(int), h->stream));
  return LMPC_OK;
}

// the polish's save area for `batch` problems of `elem`-byte values: the single-precision entry needs nothing else of
// lmpc_reserve (no fp64 workspace, no list), and half the bytes
int reserve_save(lmpc_handle* h, size_t batch, size_t elem) {
  return grow(h, h->save_cap, batch * elem, [&]() -> int {
    h->P.save = nullptr;
    HIP_TRY(h, h->save.alloc(batch * (size_t)(10 * h->P.N - 4) * elem));
    h->P.save = h->save.get();
    return LMPC_OK;
  });
}

// work area of the sequential-QP solve for up to B problems: QP solution + penalty weights, per-problem ints, a counter
int reserve_sqp(lmpc_handle* h, size_t B) {
  return grow(h, h->sqp_cap, B, [&]() -> int {
    const size_t N = (size_t)h->P.N, S = (size_t)h->P.S;
    HIP_TRY(h, h->sqp_ws.alloc((2 * (6 * N + 4 * (N - 1) + S) + 1) * B));
    HIP_TRY(h, h->sqp_int.alloc(4 * B + 1));
    if (!h->sqp_count_host.get()) HIP_TRY(h, h->sqp_count_host.alloc(1));
    return LMPC_OK;
  });
}

// every batched solve between fp64 arrays: linearise (+ regress) onto the workspace, then the QP kernel(s)
int solve_batch(lmpc_handle* h, solve_args<> a) {
  if (!h) return LMPC_ERR_ARGUMENT;
  // (total_length is not part of the request: abscissa alignment (racing_mpc.cpp:219-223) shifts s only; the QP is invariant to it)
  if (a.B < 0 || !a.x_ic || !a.u_ic || !a.X_ref || !a.U_ref || !a.T_ref || !a.bl || !a.br || !a.curv || !a.vref || !a.X || !a.U ||
      !a.dU || !a.status || !a.iters)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_solve_batch: null pointer or negative batch");
  if (const int rc = fleet_reg_batch_check(h, a.B, "lmpc_solve_batch")) return rc;
  if (h->dtrack_model && a.B != h->dtrack_B)  // (before anything is touched: problem b is linearised on vehicle b)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_solve_batch: the double-track controller model is on (lmpc_dtrack_set_controller_model) and batch " +
                                          std::to_string(a.B) + " is not the table's " + std::to_string(h->dtrack_B));
  if (h->cars_model && a.B != h->cars_B)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_solve_batch: the per-car controller model is on (lmpc_cars_set_controller_model) and batch " +
                                          std::to_string(a.B) + " is not the car table's " + std::to_string(h->cars_B));
  // A configuration the mixed entry has no kernel for (the learning problem at N >= 24, the hard hull equality) is solved in fp64
  // (round 6, VERDICT r5 item 7 / weak 10: it was LMPC_ERR_UNSUPPORTED, and a caller iterating over horizons had to special-case a
  // valid reference configuration); lmpc_last_solve_precision tells the caller which it was.
  if (a.mixed && (h->P.hard_hull || !choose_kernel(h, SOLVE_MIXED).fn)) a.mixed = false;
  h->last_precision = a.mixed ? LMPC_PRECISION_MIXED : LMPC_PRECISION_F64;
  if (h->P.learning && !a.ss_idx && (!a.ss_x || !a.ss_j)) return fail(h, LMPC_ERR_ARGUMENT, "learning=1 needs ss_x and ss_j");
  if (a.ss_idx && (!h->P.learning || !h->ss_x.get() || h->ss_laps < 1))
    return fail(h, LMPC_ERR_ARGUMENT, "ss_idx needs learning=1 and a safe set stored on the handle (lmpc_set_safe_set)");
  if (a.B == 0) return LMPC_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  if ((size_t)a.B > h->ws_cap) {
    const int rc = lmpc_reserve(h, a.B);
    if (rc != LMPC_OK) return rc;
  }
  if (h->timing) HIP_TRY(h, hipEventRecord(h->ev[0], h->stream));
  int rc = LMPC_OK;
  if (h->dtrack_model)  // the four-wheel model of car b's vehicle into the same records (include/lmpc_hip_dtrack_model.h)
    HIP_TRY(h, lmpc_dtrack_launch_linearize(h->stream, h->dtrack_tab.get(), h->P.N, a.B, true, a.X_ref, a.U_ref, a.T_ref, a.curv, h->ws.get(),
                                            nullptr, nullptr));
  else if (h->cars_model)  // the single-track model of car b's own vehicle into the same records (include/lmpc_hip_cars_model.h)
    HIP_TRY(h, lmpc_cars_launch_linearize(h->stream, h->cars_tab.get(), h->P.N, a.B, true, a.X_ref, a.U_ref, a.T_ref, a.curv, h->ws.get(), nullptr,
                                          nullptr));
  else
    rc = launch_linearize(h, a.mixed ? 4 : 8, a.B, a.X_ref, a.U_ref, a.T_ref, a.curv, h->ws.get());
  if (rc != LMPC_OK) return rc;
  if (h->reg_on) {  // error-dynamics regression onto the workspace (safe_set.cpp:182-245)
    rc = launch_regress<true>(h, a.B, a.X_ref, a.U_ref, h->ws.get(), nullptr, nullptr);
    if (rc != LMPC_OK) return rc;
  }
  if (h->freg_on) {  // the same against each car's own laps (B controllers, B SafeSetManagers)
    rc = launch_fleet_regress(h, true, a.X_ref, a.U_ref, h->ws.get(), nullptr, nullptr);
    if (rc != LMPC_OK) return rc;
  }
  if (h->timing) HIP_TRY(h, hipEventRecord(h->ev[1], h->stream));
  const launch_choice cold = choose_kernel(h, a.mixed ? SOLVE_MIXED : SOLVE_F64);
  if (!cold.fn) return fail(h, LMPC_ERR_UNSUPPORTED, "no kernel for this (N, num_ss_pts)");
  // the tracking problem takes no safe set and returns no weights; by reference, the points are not arrays
  if (!h->P.learning || a.ss_idx) a.ss_x = a.ss_j = nullptr;
  if (!h->P.learning) a.ss_idx = nullptr, a.lam = nullptr;
  // the warm start is built into fp64 kernels of its own -- the tracking problem at every horizon, the learning problem (with the
  // plan's simplex weights) up to N = 60; everywhere else the call is the cold solve it would fall back to
  const launch_choice warm = choose_kernel(h, SOLVE_WARM);
  const bool warm_built = !a.mixed && (!h->P.learning || a.warm_lam) && warm.fn;
  if (!warm_built) a.warm_X = a.warm_U = nullptr;
  if (!warm_built || !h->P.learning) a.warm_lam = nullptr;
  h->warm_flag_n = 0;  // (a cold solve: nothing was attempted)
  // Mixed precision is two launches when the polish is on: the fp32 iteration verifies its own answers (polish accepted =
  // KKT test passed) and marks the problems it could not verify -- a percent of a batch: active sets still ambiguous at
  // mu = 2e-6, or more than four free simplex weights -- and the fp64 kernel behind it solves exactly those.
  const bool two_pass = a.mixed && h->P.polish == 0;  // (polish = 1: the marks stay visible, no second pass -- diagnostics)
#ifdef LMPC_DEBUG_HOOKS  // LMPC_DEBUG_CLEANUP_ALL (the debug build, tests/second_pass_check.py): skip the fp32 pass and hand the
                         // whole batch to the fp64 second pass
  static const bool cleanup_all = getenv("LMPC_DEBUG_CLEANUP_ALL") != nullptr;
#else
  const bool cleanup_all = false;
#endif
  if (two_pass && cleanup_all)
    HIP_TRY(h, hipMemsetD32Async((hipDeviceptr_t)a.status, LMPC_SOLVE_UNVERIFIED, (size_t)a.B, h->stream));
  else if (a.warm_X && a.warm_U)
    rc = launch_solve(h, SOLVE_WARM, warm, a, h->ws.get());
  else
    rc = launch_solve(h, a.mixed ? SOLVE_MIXED : SOLVE_F64, cold, a, h->ws.get());
  if (rc != LMPC_OK) return rc;
  if (two_pass) {
    const launch_choice second = choose_kernel(h, SOLVE_SECOND_PASS);
    if (!second.fn) return fail(h, LMPC_ERR_UNSUPPORTED, "no fp64 second pass for this (N, num_ss_pts)");
    hipLaunchKernelGGL(lmpc_collect_unverified_kernel, dim3(1), dim3(1024), 0, h->stream, a.B, a.status, h->unverified.get());
    HIP_TRY(h, hipGetLastError());
    rc = launch_solve(h, SOLVE_SECOND_PASS, second, a, h->ws.get());
    if (rc != LMPC_OK) return rc;
  }
  if (h->timing) HIP_TRY(h, hipEventRecord(h->ev[2], h->stream));
  return LMPC_OK;
}

// the single-problem host entries: `r` holds HOST arrays in the reference's column-major layout; staged through the handle's pinned
// mirror into a batch of one
int solve_host(lmpc_handle* h, const solve_args<>& r) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!r.x_ic || !r.u_ic || !r.X_ref || !r.U_ref || !r.T_ref || !r.bl || !r.br || !r.curv || !r.vref || !r.X || !r.U || !r.dU ||
      !r.status || !r.iters)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_solve_host: null pointer");
  if (const int rc = fleet_reg_batch_check(h, 1, "lmpc_solve_host")) return rc;
  const int N = h->P.N, NS = N - 1, S = h->P.S;
  // staging layout (doubles): inputs then outputs, each in the batch = 1 device layout
  const size_t o_x = 0, o_u = 6, o_X = 8, o_U = o_X + 6 * N, o_T = o_U + 2 * NS, o_bl = o_T + NS, o_br = o_bl + N,
               o_k = o_br + N, o_v = o_k + N, o_sx = o_v + N, o_sj = o_sx + 6 * (size_t)S, o_Xo = o_sj + S,
               o_Uo = o_Xo + 6 * N, o_dUo = o_Uo + 2 * NS, o_lam = o_dUo + 2 * NS, o_mv = o_lam + S, o_wX = o_mv + 2, o_wU = o_wX + 6 * N,
               o_wL = o_wU + 2 * NS, total = o_wL + S;
  HIP_TRY(h, hipSetDevice(h->device));
  double* const d = h->stage_dev.get();
  double* const host = h->stage_host.get();  // pinned: the two copies below are asynchronous DMA transfers
  if (total != h->stage_doubles || !d || !host) return fail(h, LMPC_ERR_RUNTIME, "lmpc_solve_host: staging not allocated");
  for (size_t e = o_sx; e < o_Xo; ++e) host[e] = 0.0;
  for (int k = 0; k < 6; ++k) host[o_x + k] = r.x_ic[k];
  for (int k = 0; k < 2; ++k) host[o_u + k] = r.u_ic[k];
  for (int i = 0; i < N; ++i)
    for (int k = 0; k < 6; ++k) host[o_X + (size_t)k * N + i] = r.X_ref[(size_t)i * 6 + k];  // column-major -> [6][N]
  for (int i = 0; i < NS; ++i) {
    for (int k = 0; k < 2; ++k) host[o_U + (size_t)k * NS + i] = r.U_ref[(size_t)i * 2 + k];
    host[o_T + i] = r.T_ref[i];
  }
  for (int i = 0; i < N; ++i) {
    host[o_bl + i] = r.bl[i];
    host[o_br + i] = r.br[i];
    host[o_k + i] = r.curv[i];
    host[o_v + i] = r.vref[i];
  }
  if (S && r.ss_x && r.ss_j)
    for (int j = 0; j < S; ++j) {
      for (int k = 0; k < 6; ++k) host[o_sx + (size_t)k * S + j] = r.ss_x[(size_t)j * 6 + k];
      host[o_sj + j] = r.ss_j[j];
    }
  HIP_TRY(h, hipMemcpyAsync(d, host, o_Xo * sizeof(double), hipMemcpyHostToDevice, h->stream));
  const bool warm = r.warm_X && r.warm_U && r.max_sqp <= 0 && (!h->P.learning || r.warm_lam);
  if (warm) {  // the plan, column-major -> [6][N] / [2][N-1] (and, learning, its simplex weights)
    for (int i = 0; i < N; ++i)
      for (int k = 0; k < 6; ++k) host[o_wX + (size_t)k * N + i] = r.warm_X[(size_t)i * 6 + k];
    for (int i = 0; i < NS; ++i)
      for (int k = 0; k < 2; ++k) host[o_wU + (size_t)k * NS + i] = r.warm_U[(size_t)i * 2 + k];
    if (S && r.warm_lam)
      for (int j = 0; j < S; ++j) host[o_wL + j] = r.warm_lam[j];
    HIP_TRY(h, hipMemcpyAsync(d + o_wX, host + o_wX, (total - o_wX) * sizeof(double), hipMemcpyHostToDevice, h->stream));
  }
  // the same request on the staged device arrays (the staging buffer is unpacked as [6][N]: the default layout)
  int* const di = h->stage_int.get();
  solve_args<> a{1, d + o_x, d + o_u, d + o_X, d + o_U, d + o_T, d + o_bl, d + o_br, d + o_k, d + o_v, d + o_Xo, d + o_Uo, d + o_dUo, di, di + 1};
  if (S) a.ss_x = d + o_sx, a.ss_j = d + o_sj, a.lam = d + o_lam;
  if (warm) a.warm_X = d + o_wX, a.warm_U = d + o_wU;
  if (warm && S) a.warm_lam = d + o_wL;
  const int rc = r.max_sqp > 0 ? lmpc_solve_full_dynamics_batch(h, 1, a.x_ic, a.u_ic, a.X_ref, a.U_ref, a.T_ref, a.bl, a.br, a.curv, a.vref, 0.0,
                                                                a.ss_x, a.ss_j, r.max_sqp, r.step_tol, a.X, a.U, a.dU, a.lam, di, di + 1, di + 2,
                                                                d + o_mv, d + o_mv + 1)
                               : solve_batch(h, a);
  if (rc != LMPC_OK) return rc;
  int* const si = h->stage_int_host.get();
  HIP_TRY(h, hipMemcpyAsync(host + o_Xo, d + o_Xo, (o_wX - o_Xo) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipMemcpyAsync(si, di, 3 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < N; ++i)
    for (int k = 0; k < 6; ++k) r.X[(size_t)i * 6 + k] = host[o_Xo + (size_t)k * N + i];
  for (int i = 0; i < NS; ++i)
    for (int k = 0; k < 2; ++k) {
      r.U[(size_t)i * 2 + k] = host[o_Uo + (size_t)k * NS + i];
      r.dU[(size_t)i * 2 + k] = host[o_dUo + (size_t)k * NS + i];
    }
  if (S && r.lam)
    for (int j = 0; j < S; ++j) r.lam[j] = host[o_lam + j];
  *r.status = si[0];
  *r.iters = si[1];
  if (r.sqp_iters) *r.sqp_iters = r.max_sqp > 0 ? si[2] : 1;
  if (r.sqp_move) *r.sqp_move = r.max_sqp > 0 ? host[o_mv] : 0.0;
  if (r.defect) *r.defect = r.max_sqp > 0 ? host[o_mv + 1] : 0.0;
  return LMPC_OK;
}

bool track_ok(const lmpc_track* t) {
  return t && t->curvature && t->bound_left && t->bound_right && t->vel && t->M >= 2 && t->L > 0.0;
}

int prepare_impl(lmpc_handle* h, const char* who, int32_t batch, const lmpc_track* track, const double* x_ic,
                 const int32_t* status, double dt, double speed_scale, double speed_limit, double* X_ref, double* U_ref,
                 double* T_ref, double* bound_left, double* bound_right, double* curvatures, double* vel_ref) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (batch < 0 || !track_ok(track) || !x_ic || !X_ref || !U_ref || !T_ref || !bound_left || !bound_right || !curvatures || !vel_ref ||
      !(dt > 0.0))
    return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": bad argument");
  if (batch == 0) return LMPC_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(lmpc_prepare_kernel, dim3((batch + 255) / 256), dim3(256), 0, h->stream, h->P, batch, *track, x_ic,
                     status, dt, speed_scale, speed_limit, X_ref, U_ref, T_ref, bound_left, bound_right, curvatures, vel_ref);
  HIP_TRY(h, hipGetLastError());
  return LMPC_OK;
}

// what every safe-set query needs of the configuration; more than 64 points per lap is `too_many` (the fleet query refuses it as an
// argument, under its own name)
int ss_query_check(lmpc_handle* h, int too_many, const char* who) {
  if (h->cfg.num_ss_pts < 1 || h->cfg.num_ss_pts_per_lap < 1)
    return fail(h, LMPC_ERR_ARGUMENT, "num_ss_pts / num_ss_pts_per_lap not configured");
  if (h->cfg.num_ss_pts_per_lap > 64) return fail(h, too_many, std::string(who) + "num_ss_pts_per_lap > 64");
  return LMPC_OK;
}

// the shared-store query's LDS bytes: three doubles per sample of the longest lap
int ss_query_lds(lmpc_handle* h, size_t* lds) {
  *lds = (size_t)3 * (h->ss_nmax > 0 ? h->ss_nmax : 1) * sizeof(double);
  if (*lds > 160 * 1024) return fail(h, LMPC_ERR_UNSUPPORTED, "lap longer than 6826 samples");
  return LMPC_OK;
}

int ss_query_launch(lmpc_handle* h, int32_t batch, const double* query, double* ss_x, double* ss_j, int32_t* n_found, double* j0,
                    int32_t* ss_idx, size_t lds) {
  HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&lmpc_ss_query_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(lmpc_ss_query_kernel, dim3(8 * ((batch + 7) / 8)), dim3(64), lds, h->stream, batch, h->ss_laps, h->cfg.num_ss_pts,
                     h->cfg.num_ss_pts_per_lap, h->ss_npts.get(), h->ss_off.get(), h->ss_x.get(), h->ss_L, query, ss_x, ss_j, n_found, j0,
                     ss_idx);
  HIP_TRY(h, hipGetLastError());
  return LMPC_OK;
}

int ss_query_batch(lmpc_handle* h, int32_t batch, const double* query, double* ss_x, double* ss_j, int32_t* n_found, int32_t* ss_idx) {
  const int rc = ss_query_check(h, LMPC_ERR_UNSUPPORTED, "");
  if (rc != LMPC_OK) return rc;
  if (batch == 0) return LMPC_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  size_t lds = 0;
  const int rl = ss_query_lds(h, &lds);
  if (rl != LMPC_OK) return rl;
  return ss_query_launch(h, batch, query, ss_x, ss_j, n_found, nullptr, ss_idx, lds);
}

int fleet_check(lmpc_handle* h, int32_t batch, const char* who) {
  if (!h->fleet.B) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": no fleet store (lmpc_fleet_ss_create)");
  if (batch != h->fleet.B)
    return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": batch " + std::to_string(batch) + " is not the store's " + std::to_string(h->fleet.B));
  return LMPC_OK;
}

int ekf_check(lmpc_handle* h, int32_t batch, const char* who) {
  if (!h->ekf.B) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": no filter (lmpc_ekf_create)");
  if (batch != h->ekf.B)
    return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": batch " + std::to_string(batch) + " is not the filter's " + std::to_string(h->ekf.B));
  return LMPC_OK;
}

}  // namespace

extern "C" {

int lmpc_create(const lmpc_config* cfg, const lmpc_vehicle* veh, int device, lmpc_handle** out) {
  if (!cfg || !veh || !out) return LMPC_ERR_ARGUMENT;
  *out = nullptr;
  lmpc_handle* h = new (std::nothrow) lmpc_handle();
  if (!h) return LMPC_ERR_RUNTIME;
  *out = h;  // returned even on failure so that lmpc_last_error can be read; caller destroys it
  if (veh->model_id != LMPC_MODEL_SINGLE_TRACK_PLANAR)
    return fail(h, LMPC_ERR_UNSUPPORTED, "only single_track_planar_model is built (vehicle_model_factory.cpp:31-49)");
  if (cfg->N < 3 || cfg->N > 81) return fail(h, LMPC_ERR_ARGUMENT, "N must be in [3, 81]");  // (lmpc_slot_class has no class past 81)
  if (cfg->learning && (cfg->num_ss_pts < 1 || cfg->num_ss_pts_per_lap < 1))
    return fail(h, LMPC_ERR_ARGUMENT, "learning needs num_ss_pts >= 1 and num_ss_pts_per_lap >= 1");
  if (cfg->learning && ks_for(cfg->num_ss_pts) < 0)
    return fail(h, LMPC_ERR_UNSUPPORTED, "LMPC kernel is built for num_ss_pts <= 192");
  bool hard_hull = false;
  if (cfg->learning) {
    bool any = false;
    for (int k = 0; k < 6; ++k) any = any || cfg->convex_hull_slack[k] > 0.0;
    for (int k = 0; k < 6; ++k)
      if (cfg->convex_hull_slack[k] < 0.0) return fail(h, LMPC_ERR_ARGUMENT, "convex_hull_slack must be non-negative");
    // a zero component is a free slack component (racing_mpc.cpp:497-499: its cost weight is zero); ALL zero turns the
    // hull row into an equality (:500-502): the penalty limit, see LMPC_HARD_HULL_WEIGHT
    hard_hull = !any;
  }
  h->cfg = *cfg;
  h->device = device;
  lmpc_params& P = h->P;
  std::memset(&P, 0, sizeof(P));
  P.N = cfg->N;
  P.has_sigma = cfg->q_boundary > 0.0 ? 1 : 0;
  P.learning = cfg->learning ? 1 : 0;
  P.S = cfg->learning ? cfg->num_ss_pts : 0;
  P.max_iter = cfg->max_iter > 0 ? cfg->max_iter : 60;  // (40 until round 6: one problem of the benched configs[4] share needs 46 -- e_y 0.19 m outside the boundary at x_0 --, the dense oracle solves it: tests/test_gpu_spec_workload.py)
  P.polish = cfg->polish;
  P.tol = cfg->tol > 0.0 ? cfg->tol : 3e-14;
  const double qd[6] = {0.0, cfg->q_contour, cfg->q_heading, cfg->q_vel, cfg->q_vy, cfg->q_vyaw};
  const double qt[6] = {0.0, cfg->q_contour, cfg->q_heading, cfg->q_vel, 0.0, 0.0};
  for (int k = 0; k < 6; ++k) {
    P.Qd[k] = 2.0 * qd[k];
    P.Qt[k] = 20.0 * qt[k];
    P.x_max[k] = cfg->x_max[k];
    P.x_min[k] = cfg->x_min[k];
    P.chs2[k] = hard_hull ? 2.0 * LMPC_HARD_HULL_WEIGHT : 2.0 * cfg->convex_hull_slack[k];
  }
  P.hard_hull = hard_hull ? 1 : 0;
  P.qv_stage = -2.0 * cfg->q_vel;
  P.qv_term = -20.0 * cfg->q_vel;
  for (int a = 0; a < 2; ++a)
    for (int c = 0; c < 2; ++c) {
      P.Qu[a * 2 + c] = cfg->R[a * 2 + c] + cfg->R[c * 2 + a];
      P.Sv[a * 2 + c] = cfg->R_d[a * 2 + c] + cfg->R_d[c * 2 + a];
    }
  P.qsig = 2.0 * cfg->q_boundary;
  P.u_lo[0] = std::fmax(cfg->u_min[0], veh->Fb_max / 1000.0);  // single_track_planar_model.cpp:114
  P.u_hi[0] = std::fmin(cfg->u_max[0], veh->Fd_max / 1000.0);
  P.u_lo[1] = std::fmax(cfg->u_min[1], -veh->max_steer);       // :120
  P.u_hi[1] = std::fmin(cfg->u_max[1], veh->max_steer);
  P.v_lo[0] = veh->Fb_max / 1000.0 / veh->Tb;                  // :146-151
  P.v_hi[0] = veh->Fd_max / 1000.0 / veh->Td;
  P.v_lo[1] = -veh->max_steer_rate;
  P.v_hi[1] = veh->max_steer_rate;
  P.marg = cfg->margin + veh->b / 2.0;                         // racing_mpc.cpp:531
  P.max_vel_ref_diff = cfg->max_vel_ref_diff;
  P.veh = *veh;
  if (!(P.Sv[0] > 0.0) || !(P.Sv[0] * P.Sv[3] - P.Sv[1] * P.Sv[2] > 0.0))
    return fail(h, LMPC_ERR_ARGUMENT, "R_d must be positive definite");
  HIP_TRY(h, hipSetDevice(device));
  for (auto& e : h->ev) HIP_TRY(h, hipEventCreate(&e));
  {  // staging of the single-problem host path, once
    const size_t N = (size_t)P.N, S = (size_t)P.S;
    h->stage_doubles = 8 + 6 * N + 2 * (N - 1) + (N - 1) + 4 * N + 7 * S + 6 * N + 4 * (N - 1) + S + 2 + 6 * N + 2 * (N - 1) + S;  // (+ a warm plan and its simplex weights)
    HIP_TRY(h, h->stage_dev.alloc(h->stage_doubles));
    HIP_TRY(h, h->stage_host.alloc(h->stage_doubles));
    HIP_TRY(h, h->stage_int.alloc(3));
    HIP_TRY(h, h->stage_int_host.alloc(3));
    if (cfg->num_ss_pts >= 1) {
      const size_t nd = 2 + 7 * (size_t)cfg->num_ss_pts + 1;
      HIP_TRY(h, h->ssq_dev.alloc(nd));
      HIP_TRY(h, h->ssq_host.alloc(nd));
      HIP_TRY(h, h->ssq_int.alloc(1));
      HIP_TRY(h, h->ssq_int_host.alloc(1));
    }
    int rc = lmpc_reserve(h, 1);
    if (rc == LMPC_OK) rc = reserve_sqp(h, 1);
    if (rc != LMPC_OK) return rc;
  }
  // what the device holds of the warm kernel at once (the default of lmpc_set_warm_rounds goes by it)
  if (const launch_choice warm = choose_kernel(h, SOLVE_WARM); warm.fn) {
    int per_cu = 0, cus = 0;
    const int rc = residency(h, warm, &per_cu);
    if (rc != LMPC_OK) return rc;
    HIP_TRY(h, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    h->warm_resident = per_cu * cus;
  }
  return LMPC_OK;
}

void lmpc_destroy(lmpc_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  delete h;  // the owners free what the handle holds
}

const char* lmpc_last_error(const lmpc_handle* h) { return h ? h->err.c_str() : "null handle"; }

int lmpc_set_stream(lmpc_handle* h, void* hip_stream) {
  if (!h) return LMPC_ERR_ARGUMENT;
  h->stream = reinterpret_cast<hipStream_t>(hip_stream);
  return LMPC_OK;
}

int lmpc_synchronize(lmpc_handle* h) {
  if (!h) return LMPC_ERR_ARGUMENT;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return LMPC_OK;
}

int lmpc_reserve(lmpc_handle* h, int32_t max_batch) {
  if (!h || max_batch < 0) return LMPC_ERR_ARGUMENT;
  if ((size_t)max_batch <= h->ws_cap) return LMPC_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t B = (size_t)max_batch;
  return grow(h, h->ws_cap, B, [&]() -> int {
    HIP_TRY(h, h->ws.alloc(B * (h->P.N - 1) * LMPC_LIN_RECORD));
    HIP_TRY(h, h->unverified.alloc(B + 1));
    h->warm_flag_n = 0;
    HIP_TRY(h, h->warm_flag.alloc(B));
    // the polish's save area belongs to it: a batch counts as reserved only when everything a solve of that size touches exists
    // (with ws_cap set before a failed reserve_save a later solve skipped the reservation and wrote through a null save)
    return reserve_save(h, B, sizeof(double));
  });
}

int lmpc_query_launch(const lmpc_handle* h, int32_t* lds_bytes_per_problem, int32_t* threads_per_problem) {
  if (!h) return LMPC_ERR_ARGUMENT;
  // (two wavefronts per problem where the cold fp64 tracking solve takes those kernels: lmpc_set_waves_per_problem)
  const launch_choice k = choose_kernel(h, SOLVE_F64);
  if (lds_bytes_per_problem) *lds_bytes_per_problem = (int32_t)k.lds;
  if (threads_per_problem) *threads_per_problem = k.threads;
  return LMPC_OK;
}

int lmpc_query_residency(lmpc_handle* h, int32_t* problems_per_cu) {
  if (!h || !problems_per_cu) return LMPC_ERR_ARGUMENT;
  HIP_TRY(h, hipSetDevice(h->device));
  const launch_choice k = choose_kernel(h, SOLVE_F64_ONE_WAVE);
  if (!k.fn) return fail(h, LMPC_ERR_UNSUPPORTED, "no kernel for this (N, num_ss_pts)");
  int n = 0;
  const int rc = residency(h, k, &n);
  if (rc == LMPC_OK) *problems_per_cu = n;
  return rc;
}

int lmpc_query_launch_for(lmpc_handle* h, int32_t precision, int32_t* lds_bytes_per_problem, int32_t* problems_per_cu) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (precision != LMPC_PRECISION_F64 && precision != LMPC_PRECISION_F32 && precision != LMPC_PRECISION_MIXED)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_query_launch_for: unknown precision");
  HIP_TRY(h, hipSetDevice(h->device));
  // (what the entry point of that precision launches for this handle: the fp64 one possibly two wavefronts per problem)
  const launch_choice k = choose_kernel(h, precision == LMPC_PRECISION_F64 ? SOLVE_F64 : precision == LMPC_PRECISION_MIXED ? SOLVE_MIXED : SOLVE_F32);
  if (!k.fn) return fail(h, LMPC_ERR_UNSUPPORTED, "no kernel for this (N, num_ss_pts) at this precision");
  if (lds_bytes_per_problem) *lds_bytes_per_problem = (int32_t)k.lds;
  if (problems_per_cu) {
    int n = 0;
    const int rc = residency(h, k, &n);
    if (rc != LMPC_OK) return rc;
    *problems_per_cu = n;
  }
  return LMPC_OK;
}

int lmpc_set_waves_per_problem(lmpc_handle* h, int32_t waves) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (waves < 0 || waves > 2) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_set_waves_per_problem: 0 (the library's choice), 1 or 2");
  h->waves = waves;
  return LMPC_OK;
}

int lmpc_last_solve_precision(const lmpc_handle* h, int32_t* precision) {
  if (!h || !precision) return LMPC_ERR_ARGUMENT;
  *precision = h->last_precision;
  return LMPC_OK;
}

int lmpc_enable_timing(lmpc_handle* h, int32_t on) {
  if (!h) return LMPC_ERR_ARGUMENT;
  h->timing = on != 0;
  return LMPC_OK;
}

int lmpc_last_kernel_ms(lmpc_handle* h, float* linearize_ms, float* solve_ms) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!h->timing) return fail(h, LMPC_ERR_ARGUMENT, "timing not enabled");
  HIP_TRY(h, hipEventSynchronize(h->ev[2]));
  float a = 0.f, b = 0.f;
  HIP_TRY(h, hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
  HIP_TRY(h, hipEventElapsedTime(&b, h->ev[1], h->ev[2]));
  if (linearize_ms) *linearize_ms = a;
  if (solve_ms) *solve_ms = b;
  return LMPC_OK;
}

int lmpc_linearize_batch(lmpc_handle* h, int32_t batch, const double* X_ref, const double* U_ref, const double* T_ref,
                         const double* curvatures, double* A, double* Bm, double* g) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (batch < 0 || !X_ref || !U_ref || !T_ref || !curvatures || !A || !Bm || !g)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_linearize_batch: null pointer or negative batch");
  if (batch == 0) return LMPC_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  dim3 grid((batch + 255) / 256, h->P.N - 1);
  hipLaunchKernelGGL((lmpc_linearize_kernel<false, double, 1>), grid, dim3(256), 0, h->stream, h->P, batch, X_ref, U_ref, T_ref,
                     curvatures, A, Bm, g);
  HIP_TRY(h, hipGetLastError());
  return LMPC_OK;
}

int lmpc_solve_batch(lmpc_handle* h, int32_t batch, const double* x_ic, const double* u_ic, const double* X_ref,
                     const double* U_ref, const double* T_ref, const double* bound_left, const double* bound_right,
                     const double* curvatures, const double* vel_ref, double total_length, const double* ss_x,
                     const double* ss_j, double* X_optm, double* U_optm, double* dU_optm, double* convex_combi_optm,
                     int32_t* status, int32_t* iters, double* kkt) {
  solve_args<> a{batch, x_ic, u_ic, X_ref, U_ref, T_ref, bound_left, bound_right, curvatures, vel_ref, X_optm, U_optm, dU_optm, status, iters, kkt};
  a.ss_x = ss_x, a.ss_j = ss_j, a.lam = convex_combi_optm;
  a.aos = h && h->out_aos;
  return solve_batch(h, a);
}

int lmpc_solve_batch_mixed(lmpc_handle* h, int32_t batch, const double* x_ic, const double* u_ic, const double* X_ref,
                           const double* U_ref, const double* T_ref, const double* bound_left, const double* bound_right,
                           const double* curvatures, const double* vel_ref, double total_length, const double* ss_x,
                           const double* ss_j, double* X_optm, double* U_optm, double* dU_optm,
                           double* convex_combi_optm, int32_t* status, int32_t* iters, double* kkt) {
  solve_args<> a{batch, x_ic, u_ic, X_ref, U_ref, T_ref, bound_left, bound_right, curvatures, vel_ref, X_optm, U_optm, dU_optm, status, iters, kkt};
  a.ss_x = ss_x, a.ss_j = ss_j, a.lam = convex_combi_optm;
  a.mixed = true;
  a.aos = h && h->out_aos;
  return solve_batch(h, a);
}

int lmpc_solve_batch_warm(lmpc_handle* h, int32_t batch, const double* x_ic, const double* u_ic, const double* X_ref, const double* U_ref,
                          const double* T_ref, const double* bound_left, const double* bound_right, const double* curvatures,
                          const double* vel_ref, double total_length, const double* X_optm_ref, const double* U_optm_ref, double* X_optm,
                          double* U_optm, double* dU_optm, int32_t* status, int32_t* iters, double* kkt) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!X_optm_ref || !U_optm_ref) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_solve_batch_warm: X_optm_ref / U_optm_ref is null");
  if (h->P.learning) return fail(h, LMPC_ERR_UNSUPPORTED, "lmpc_solve_batch_warm: the tracking problem only (learning handles: lmpc_solve_batch_warm_ss)");
  solve_args<> a{batch, x_ic, u_ic, X_ref, U_ref, T_ref, bound_left, bound_right, curvatures, vel_ref, X_optm, U_optm, dU_optm, status, iters, kkt};
  a.warm_X = X_optm_ref, a.warm_U = U_optm_ref;
  a.aos = h->out_aos;
  return solve_batch(h, a);
}

int lmpc_solve_batch_warm_ss(lmpc_handle* h, int32_t batch, const double* x_ic, const double* u_ic, const double* X_ref, const double* U_ref,
                             const double* T_ref, const double* bound_left, const double* bound_right, const double* curvatures,
                             const double* vel_ref, double total_length, const double* ss_x, const double* ss_j, const int32_t* ss_idx,
                             const double* X_optm_ref, const double* U_optm_ref, const double* convex_combi_optm_ref, double* X_optm,
                             double* U_optm, double* dU_optm, double* convex_combi_optm, int32_t* status, int32_t* iters, double* kkt) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!X_optm_ref || !U_optm_ref) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_solve_batch_warm_ss: X_optm_ref / U_optm_ref is null");
  if (!h->P.learning) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_solve_batch_warm_ss: a learning handle (the tracking problem: lmpc_solve_batch_warm)");
  if (ss_idx && h->ss_idx_gen != h->ss_gen)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_solve_batch_warm_ss: the safe set was replaced (lmpc_set_safe_set) after the lmpc_ss_query_idx_batch these "
                                      "codes come from, or no such query ran on this handle");
  solve_args<> a{batch, x_ic, u_ic, X_ref, U_ref, T_ref, bound_left, bound_right, curvatures, vel_ref, X_optm, U_optm, dU_optm, status, iters, kkt};
  a.ss_x = ss_x, a.ss_j = ss_j, a.ss_idx = ss_idx, a.lam = convex_combi_optm;
  a.warm_X = X_optm_ref, a.warm_U = U_optm_ref, a.warm_lam = convex_combi_optm_ref;
  a.aos = h->out_aos;
  return solve_batch(h, a);
}

int lmpc_get_warm_accepted(lmpc_handle* h, int32_t batch, int32_t* accepted) {
  if (!h || !accepted || batch < 0) return h ? fail(h, LMPC_ERR_ARGUMENT, "lmpc_get_warm_accepted: null pointer or negative batch") : LMPC_ERR_ARGUMENT;
  if (batch == 0) return LMPC_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  if (h->warm_flag_n != batch) {  // the last solve of this size was not a warm one (or the kernel for it is not built): nothing was attempted
    HIP_TRY(h, hipMemsetAsync(accepted, 0, (size_t)batch * sizeof(int32_t), h->stream));
    return LMPC_OK;
  }
  HIP_TRY(h, hipMemcpyAsync(accepted, h->warm_flag.get(), (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
  return LMPC_OK;
}

int lmpc_shift_lambda_batch(lmpc_handle* h, int32_t batch, const int32_t* ss_idx_prev, const double* lambda_prev, const int32_t* ss_idx,
                            int32_t advance, double* lambda_ref) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (batch < 0 || !ss_idx_prev || !lambda_prev || !ss_idx || !lambda_ref || advance < 0)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_shift_lambda_batch: null pointer, negative batch or negative advance");
  if (!h->P.learning || h->ss_laps < 1) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_shift_lambda_batch: a learning handle with a safe set stored");
  if (batch == 0) return LMPC_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(lmpc_shift_lambda_kernel, dim3((batch + 63) / 64), dim3(64), 0, h->stream, batch, h->P.S, h->ss_laps, h->ss_total,
                     h->ss_npts.get(), h->ss_off.get(), ss_idx_prev, lambda_prev, ss_idx, advance, lambda_ref);
  HIP_TRY(h, hipGetLastError());
  return LMPC_OK;
}

int lmpc_solve_batch_ss_idx(lmpc_handle* h, int32_t batch, int32_t precision, const double* x_ic, const double* u_ic, const double* X_ref,
                            const double* U_ref, const double* T_ref, const double* bound_left, const double* bound_right,
                            const double* curvatures, const double* vel_ref, double total_length, const int32_t* ss_idx, double* X_optm,
                            double* U_optm, double* dU_optm, double* convex_combi_optm, int32_t* status, int32_t* iters, double* kkt) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!ss_idx) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_solve_batch_ss_idx: ss_idx is null");
  if (precision != LMPC_PRECISION_F64 && precision != LMPC_PRECISION_MIXED)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_solve_batch_ss_idx: precision is LMPC_PRECISION_F64 or LMPC_PRECISION_MIXED");
  // the codes name rows of the store the query ran against: a store replaced since -- possibly by a smaller one -- would
  // be read out of bounds, or, in bounds, silently solve on other points with status OPTIMAL
  if (h->ss_idx_gen != h->ss_gen)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_solve_batch_ss_idx: the safe set was replaced (lmpc_set_safe_set) after the lmpc_ss_query_idx_batch these "
                                      "codes come from, or no such query ran on this handle");
  solve_args<> a{batch, x_ic, u_ic, X_ref, U_ref, T_ref, bound_left, bound_right, curvatures, vel_ref, X_optm, U_optm, dU_optm, status, iters, kkt};
  a.ss_idx = ss_idx, a.lam = convex_combi_optm;
  a.mixed = precision == LMPC_PRECISION_MIXED;
  a.aos = h->out_aos;
  return solve_batch(h, a);
}

int lmpc_solve_batch_f32(lmpc_handle* h, int32_t batch, const float* x_ic, const float* u_ic, const float* X_ref,
                         const float* U_ref, const float* T_ref, const float* bound_left, const float* bound_right,
                         const float* curvatures, const float* vel_ref, float* X_optm, float* U_optm, float* dU_optm,
                         int32_t* status, int32_t* iters, float* kkt) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (batch < 0 || !x_ic || !u_ic || !X_ref || !U_ref || !T_ref || !bound_left || !bound_right || !curvatures ||
      !vel_ref || !X_optm || !U_optm || !dU_optm || !status || !iters)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_solve_batch_f32: null pointer or negative batch");
  if (h->P.learning) return fail(h, LMPC_ERR_UNSUPPORTED, "single precision is built for the tracking problem only");
  if (h->reg_on) return fail(h, LMPC_ERR_UNSUPPORTED, "the error-dynamics regression is applied in double precision only");
  if (h->freg_on) return fail(h, LMPC_ERR_UNSUPPORTED, "the per-car error-dynamics regression is applied in double precision only");
  if (h->dtrack_model)
    return fail(h, LMPC_ERR_UNSUPPORTED, "lmpc_solve_batch_f32: the double-track controller model is linearised in double precision only");
  if (h->cars_model && batch != h->cars_B)  // (before anything is touched: problem b is linearised on vehicle b)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_solve_batch_f32: the per-car controller model is on (lmpc_cars_set_controller_model) and batch " +
                                          std::to_string(batch) + " is not the car table's " + std::to_string(h->cars_B));
  if (batch == 0) return LMPC_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  const launch_choice k = choose_kernel(h, SOLVE_F32);
  if (!k.fn) return fail(h, LMPC_ERR_UNSUPPORTED, "no single-precision kernel for this N");
  h->last_precision = LMPC_PRECISION_F32;
  h->warm_flag_n = 0;  // (a cold solve, like lmpc_solve_batch's: the flags of an earlier warm solve of this batch size no longer describe the last solve)
  int rc = reserve_save(h, (size_t)batch, sizeof(float));
  if (rc == LMPC_OK)
    rc = grow(h, h->ws_f32_cap, (size_t)batch, [&]() -> int {
      HIP_TRY(h, h->ws_f32.alloc((size_t)batch * (h->P.N - 1) * LMPC_LIN_RECORD));
      return LMPC_OK;
    });
  if (rc != LMPC_OK) return rc;
  if (h->timing) HIP_TRY(h, hipEventRecord(h->ev[0], h->stream));
  if (h->cars_model)  // (include/lmpc_hip_cars_model.h: the io = float instantiation, fp64 arithmetic on car b's vehicle)
    HIP_TRY(h, lmpc_cars_launch_linearize_f32(h->stream, h->cars_tab.get(), h->P.N, batch, X_ref, U_ref, T_ref, curvatures, h->ws_f32.get()));
  else
    rc = launch_linearize(h, 4, batch, X_ref, U_ref, T_ref, curvatures, h->ws_f32.get());
  if (rc != LMPC_OK) return rc;
  if (h->timing) HIP_TRY(h, hipEventRecord(h->ev[1], h->stream));
  const solve_args<float> a{batch, x_ic, u_ic, X_ref, U_ref, T_ref, bound_left, bound_right, curvatures, vel_ref, X_optm, U_optm, dU_optm, status, iters, kkt};
  rc = launch_solve(h, SOLVE_F32, k, a, h->ws_f32.get());
  if (rc != LMPC_OK) return rc;
  if (h->timing) HIP_TRY(h, hipEventRecord(h->ev[2], h->stream));
  return LMPC_OK;
}

int lmpc_solve_full_dynamics_batch(lmpc_handle* h, int32_t batch, const double* x_ic, const double* u_ic, const double* X_ref,
                                   const double* U_ref, const double* T_ref, const double* bound_left,
                                   const double* bound_right, const double* curvatures, const double* vel_ref,
                                   double total_length, const double* ss_x, const double* ss_j, int32_t max_sqp,
                                   double step_tol, double* X_optm, double* U_optm, double* dU_optm,
                                   double* convex_combi_optm, int32_t* status, int32_t* iters, int32_t* sqp_iters,
                                   double* sqp_move, double* defect) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (batch < 0 || !X_ref || !U_ref || !X_optm || !U_optm || !dU_optm || !status || !iters || !sqp_iters || !sqp_move || !defect)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_solve_full_dynamics_batch: null pointer or negative batch");
  if (max_sqp < 1) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_solve_full_dynamics_batch: max_sqp < 1");
  if (h->dtrack_model)  // (its defects and merit are the single-track model's: a handle corrects one model)
    return fail(h, LMPC_ERR_UNSUPPORTED, "lmpc_solve_full_dynamics_batch: not built on the double-track controller model (lmpc_dtrack_set_controller_model)");
  if (h->cars_model)  // (the line search of lmpc_sqp_kernel.hip evaluates its defects on the handle's vehicle)
    return fail(h, LMPC_ERR_UNSUPPORTED, "lmpc_solve_full_dynamics_batch: not built on the per-car controller model (lmpc_cars_set_controller_model)");
  if (h->P.learning && !convex_combi_optm) return fail(h, LMPC_ERR_ARGUMENT, "learning=1 needs convex_combi_optm");
  // (solve_batch refuses this too, but only after the outputs below have been overwritten with the start)
  if (h->P.learning && (!ss_x || !ss_j)) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_solve_full_dynamics_batch: learning=1 needs ss_x and ss_j");
  if (const int rc = fleet_reg_batch_check(h, batch, "lmpc_solve_full_dynamics_batch")) return rc;
  if (batch == 0) return LMPC_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t B = (size_t)batch, N = (size_t)h->P.N, NS = N - 1, S = (size_t)h->P.S;
  const size_t nX = 6 * N * B, nU = 2 * NS * B, nL = S * B;
  // work area: QP solution (Xq, Uq, dUq, lamq), the iterate before the last step (Xp, Up, dUp, lamp), penalty weights;
  // ints: status_q, iters_q, active, consecutive back-offs, counter
  {
    const int rc = reserve_sqp(h, B);
    if (rc != LMPC_OK) return rc;
  }
  double* Xq = h->sqp_ws.get();
  double* Uq = Xq + nX;
  double* dUq = Uq + nU;
  double* lamq = dUq + nU;
  double* Xp = lamq + nL;
  double* Up = Xp + nX;
  double* dUp = Up + nU;
  double* lamp = dUp + nU;
  double* nu = lamp + nL;
  int* status_q = h->sqp_int.get();
  int* iters_q = status_q + B;
  int* active = iters_q + B;
  int* backoffs = active + B;
  int* counter = backoffs + B;
  int* const count_host = h->sqp_count_host.get();
  // the iterate lives in the caller's output arrays: start = the reference trajectory (the node's zero-input rollout,
  // racing_mpc_node.cpp:210-235), dU = 0, lambda = 0 (its convex_combi_optm_ref)
  HIP_TRY(h, hipMemcpyAsync(X_optm, X_ref, nX * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(U_optm, U_ref, nU * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  HIP_TRY(h, hipMemsetAsync(dU_optm, 0, nU * sizeof(double), h->stream));
  if (S) HIP_TRY(h, hipMemsetAsync(convex_combi_optm, 0, nL * sizeof(double), h->stream));
  HIP_TRY(h, hipMemsetAsync(nu, 0, B * sizeof(double), h->stream));
  HIP_TRY(h, hipMemsetAsync(backoffs, 0, B * sizeof(int), h->stream));
  HIP_TRY(h, hipMemsetAsync(iters, 0, B * sizeof(int), h->stream));
  HIP_TRY(h, hipMemsetAsync(sqp_iters, 0, B * sizeof(int), h->stream));
  HIP_TRY(h, hipMemsetAsync(defect, 0, B * sizeof(double), h->stream));
  {  // active = 1, move = inf
    std::vector<int> ones(B, 1);
    std::vector<double> inf(B, INFINITY);
    HIP_TRY(h, hipMemcpyAsync(active, ones.data(), B * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(sqp_move, inf.data(), B * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  lmpc_sqp_arrays A{};
  A.X = X_optm; A.U = U_optm; A.dU = dU_optm; A.lam = S ? convex_combi_optm : nullptr;
  A.Xq = Xq; A.Uq = Uq; A.dUq = dUq; A.lamq = S ? lamq : nullptr;
  A.Xp = Xp; A.Up = Up; A.dUp = dUp; A.lamp = S ? lamp : nullptr;
  A.backoffs = backoffs; A.iters_q = iters_q; A.iters = iters;
  A.status_q = status_q;
  A.T_ref = T_ref; A.curv = curvatures; A.bl = bound_left; A.br = bound_right; A.vref = vel_ref; A.ss_x = ss_x; A.ss_j = ss_j;
  A.nu = nu; A.active = active; A.status = status; A.sqp_iters = sqp_iters; A.move = sqp_move; A.defect = defect;
  A.n_active = counter;
  // QP about the iterate (racing_mpc.cpp:169-186 with X_ref, U_ref := the iterate)
  // (the default layout whatever lmpc_set_output_layout says: the line search and the next linearisation index it)
  solve_args<> qp{batch, x_ic, u_ic, X_optm, U_optm, T_ref, bound_left, bound_right, curvatures, vel_ref, Xq, Uq, dUq, status_q, iters_q};
  qp.ss_x = ss_x, qp.ss_j = ss_j, qp.lam = S ? lamq : nullptr;
  for (int it = 0; it < max_sqp; ++it) {
    const int rc = solve_batch(h, qp);
    if (rc != LMPC_OK) return rc;
    HIP_TRY(h, hipMemsetAsync(counter, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(lmpc_sqp_linesearch_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, h->stream, h->P, batch, A,
                       it == 0 ? 1 : 0, step_tol);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(count_host, counter, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (*count_host == 0) break;
  }
  return LMPC_OK;
}

int lmpc_solve_host(lmpc_handle* h, const double* x_ic, const double* u_ic, const double* X_ref, const double* U_ref,
                    const double* T_ref, const double* bound_left, const double* bound_right, const double* curvatures,
                    const double* vel_ref, double total_length, const double* ss_x, const double* ss_j, double* X_optm,
                    double* U_optm, double* dU_optm, double* convex_combi_optm, int32_t* status, int32_t* iters) {
  solve_args<> r{1, x_ic, u_ic, X_ref, U_ref, T_ref, bound_left, bound_right, curvatures, vel_ref, X_optm, U_optm, dU_optm, status, iters};
  r.ss_x = ss_x, r.ss_j = ss_j, r.lam = convex_combi_optm;
  return solve_host(h, r);
}

int lmpc_solve_host_warm(lmpc_handle* h, const double* x_ic, const double* u_ic, const double* X_ref, const double* U_ref,
                         const double* T_ref, const double* bound_left, const double* bound_right, const double* curvatures,
                         const double* vel_ref, double total_length, const double* X_optm_ref, const double* U_optm_ref, double* X_optm,
                         double* U_optm, double* dU_optm, int32_t* status, int32_t* iters) {
  if (h && (!X_optm_ref || !U_optm_ref)) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_solve_host_warm: X_optm_ref / U_optm_ref is null");
  if (h && h->P.learning) return fail(h, LMPC_ERR_UNSUPPORTED, "lmpc_solve_host_warm: the tracking problem only (learning handles: lmpc_solve_host_warm_ss)");
  solve_args<> r{1, x_ic, u_ic, X_ref, U_ref, T_ref, bound_left, bound_right, curvatures, vel_ref, X_optm, U_optm, dU_optm, status, iters};
  r.warm_X = X_optm_ref, r.warm_U = U_optm_ref;
  return solve_host(h, r);
}

int lmpc_solve_host_warm_ss(lmpc_handle* h, const double* x_ic, const double* u_ic, const double* X_ref, const double* U_ref,
                            const double* T_ref, const double* bound_left, const double* bound_right, const double* curvatures,
                            const double* vel_ref, double total_length, const double* ss_x, const double* ss_j, const double* X_optm_ref,
                            const double* U_optm_ref, const double* convex_combi_optm_ref, double* X_optm, double* U_optm, double* dU_optm,
                            double* convex_combi_optm, int32_t* status, int32_t* iters) {
  if (h && (!X_optm_ref || !U_optm_ref || !convex_combi_optm_ref))
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_solve_host_warm_ss: X_optm_ref / U_optm_ref / convex_combi_optm_ref is null");
  if (h && !h->P.learning) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_solve_host_warm_ss: a learning handle (the tracking problem: lmpc_solve_host_warm)");
  solve_args<> r{1, x_ic, u_ic, X_ref, U_ref, T_ref, bound_left, bound_right, curvatures, vel_ref, X_optm, U_optm, dU_optm, status, iters};
  r.ss_x = ss_x, r.ss_j = ss_j, r.lam = convex_combi_optm;
  r.warm_X = X_optm_ref, r.warm_U = U_optm_ref, r.warm_lam = convex_combi_optm_ref;
  return solve_host(h, r);
}

int lmpc_solve_full_dynamics_host(lmpc_handle* h, const double* x_ic, const double* u_ic, const double* X_ref,
                                  const double* U_ref, const double* T_ref, const double* bound_left,
                                  const double* bound_right, const double* curvatures, const double* vel_ref,
                                  double total_length, const double* ss_x, const double* ss_j, int32_t max_sqp,
                                  double step_tol, double* X_optm, double* U_optm, double* dU_optm,
                                  double* convex_combi_optm, int32_t* status, int32_t* iters, int32_t* sqp_iters,
                                  double* sqp_move, double* defect) {
  if (max_sqp < 1) return h ? fail(h, LMPC_ERR_ARGUMENT, "lmpc_solve_full_dynamics_host: max_sqp < 1") : LMPC_ERR_ARGUMENT;
  solve_args<> r{1, x_ic, u_ic, X_ref, U_ref, T_ref, bound_left, bound_right, curvatures, vel_ref, X_optm, U_optm, dU_optm, status, iters};
  r.ss_x = ss_x, r.ss_j = ss_j, r.lam = convex_combi_optm;
  r.max_sqp = max_sqp, r.step_tol = step_tol, r.sqp_iters = sqp_iters, r.sqp_move = sqp_move, r.defect = defect;
  return solve_host(h, r);
}

int lmpc_prepare_batch(lmpc_handle* h, int32_t batch, const lmpc_track* track, const double* x_ic, double dt,
                       double speed_scale, double speed_limit, double* X_ref, double* U_ref, double* T_ref,
                       double* bound_left, double* bound_right, double* curvatures, double* vel_ref) {
  return prepare_impl(h, "lmpc_prepare_batch", batch, track, x_ic, nullptr, dt, speed_scale, speed_limit, X_ref, U_ref,
                      T_ref, bound_left, bound_right, curvatures, vel_ref);
}

int lmpc_prepare_failed_batch(lmpc_handle* h, int32_t batch, const lmpc_track* track, const double* x_ic,
                              const int32_t* status, double dt, double speed_scale, double speed_limit, double* X_ref,
                              double* U_ref, double* T_ref, double* bound_left, double* bound_right, double* curvatures,
                              double* vel_ref) {
  if (h && !status) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_prepare_failed_batch: status is NULL");
  return prepare_impl(h, "lmpc_prepare_failed_batch", batch, track, x_ic, status, dt, speed_scale, speed_limit, X_ref,
                      U_ref, T_ref, bound_left, bound_right, curvatures, vel_ref);
}

int lmpc_shift_batch(lmpc_handle* h, int32_t batch, const lmpc_track* track, const double* X_sol, const double* U_sol,
                     const double* X_old, const double* U_old, const int32_t* status, double dt, double speed_scale,
                     double speed_limit, double* X_ref, double* U_ref, double* T_ref, double* bound_left,
                     double* bound_right, double* curvatures, double* vel_ref) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (batch < 0 || !track_ok(track) || !X_sol || !U_sol || !X_ref || !U_ref || !T_ref || !bound_left || !bound_right ||
      !curvatures || !vel_ref || !(dt > 0.0) || (status && (!X_old || !U_old)))
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_shift_batch: bad argument");
  if (X_ref == X_sol || X_ref == X_old || U_ref == U_sol || U_ref == U_old)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_shift_batch: outputs must not alias inputs");
  if (batch == 0) return LMPC_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(lmpc_shift_kernel, dim3((batch + 255) / 256), dim3(256), 0, h->stream, h->P, batch, *track, X_sol,
                     U_sol, X_old ? X_old : X_sol, U_old ? U_old : U_sol, status, dt, speed_scale, speed_limit, X_ref,
                     U_ref, T_ref, bound_left, bound_right, curvatures, vel_ref);
  HIP_TRY(h, hipGetLastError());
  return LMPC_OK;
}

int lmpc_plant_step_batch(lmpc_handle* h, int32_t batch, const lmpc_track* track, double* x, const double* u,
                          double dt_sim, int32_t n_sub) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (batch < 0 || !track_ok(track) || !x || !u || !(dt_sim > 0.0) || n_sub < 1)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_plant_step_batch: bad argument");
  if (batch == 0) return LMPC_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(lmpc_plant_kernel, dim3((batch + 255) / 256), dim3(256), 0, h->stream, h->P, batch, *track, x, u,
                     dt_sim, n_sub);
  HIP_TRY(h, hipGetLastError());
  return LMPC_OK;
}

int lmpc_loop_advance_batch(lmpc_handle* h, int32_t batch, const lmpc_track* track, const int32_t* status, const int32_t* iters,
                            const double* X_optm, const double* U_optm, double* x, double* u_prev, double dt, double dt_sim, int32_t n_sub,
                            double speed_scale, double speed_limit, int32_t restart_failed, double* X_ref, double* U_ref, double* T_ref,
                            double* bound_left, double* bound_right, double* curvatures, double* vel_ref, double* distance,
                            double* worst_excess, int64_t* n_fail, uint64_t* n_accepted) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (batch < 0 || !track_ok(track) || !status || !X_optm || !U_optm || !x || !u_prev || !X_ref || !U_ref || !T_ref || !bound_left ||
      !bound_right || !curvatures || !vel_ref || !(dt > 0.0) || !(dt_sim > 0.0) || n_sub < 1 || (n_accepted && !iters))
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_loop_advance_batch: bad argument");
  if (X_ref == X_optm || U_ref == U_optm) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_loop_advance_batch: the references must not alias the solution");
  if (h->out_aos) return fail(h, LMPC_ERR_UNSUPPORTED, "lmpc_loop_advance_batch reads the solution in the [component][knot][batch] layout");
  if (batch == 0) return LMPC_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(unsigned long long) == sizeof(uint64_t), "counter types");
  lmpc_params PL = h->P;
  PL.warm_flag = (h->warm_flag.get() && h->warm_flag_n == batch) ? h->warm_flag.get() : nullptr;  // the last solve of this batch was a warm one
  hipLaunchKernelGGL(lmpc_loop_advance_kernel, dim3((batch + 63) / 64), dim3(64 * lmpc_loop_waves), 0, h->stream, PL, batch, *track, status, iters, X_optm,
                     U_optm, x, u_prev, dt, dt_sim, n_sub, speed_scale, speed_limit, restart_failed ? 1 : 0, X_ref, U_ref, T_ref, bound_left,
                     bound_right, curvatures, vel_ref, distance, worst_excess, reinterpret_cast<long long*>(n_fail),
                     reinterpret_cast<unsigned long long*>(n_accepted));
  HIP_TRY(h, hipGetLastError());
  return LMPC_OK;
}

int lmpc_set_safe_set(lmpc_handle* h, int32_t n_laps, const int32_t* n_pts, const double* x, double total_length) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (n_laps < 0 || (n_laps > 0 && (!n_pts || !x)) || !(total_length > 0.0))
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_set_safe_set: bad argument");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->ss_npts.release();
  h->ss_off.release();
  h->ss_x.release();
  h->ss_laps = 0;
  h->ss_total = 0;
  h->ss_nmax = 0;
  h->ss_L = total_length;
  ++h->ss_gen;  // codes of an earlier lmpc_ss_query_idx_batch no longer name rows of this store (lmpc_solve_batch_ss_idx refuses them)
  // SafeSetManager keeps at most max_lap_stored laps (boost::circular_buffer, safe_set.cpp:139-151)
  int first = 0;
  if (h->cfg.max_lap_stored > 0 && n_laps > h->cfg.max_lap_stored) first = n_laps - h->cfg.max_lap_stored;
  std::vector<int> npts, off;
  size_t skip = 0, total = 0;
  for (int l = 0; l < n_laps; ++l) {
    if (n_pts[l] < 1) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_set_safe_set: empty lap");
    if (l < first) {
      skip += (size_t)n_pts[l];
      continue;
    }
    off.push_back((int)total);
    npts.push_back(n_pts[l]);
    if (n_pts[l] > h->ss_nmax) h->ss_nmax = n_pts[l];
    total += (size_t)n_pts[l];
  }
  if (npts.empty()) return LMPC_OK;
  HIP_TRY(h, h->ss_npts.alloc(npts.size()));
  HIP_TRY(h, h->ss_off.alloc(off.size()));
  HIP_TRY(h, h->ss_x.alloc(total * 6));
  HIP_TRY(h, hipMemcpy(h->ss_npts.get(), npts.data(), npts.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(h, hipMemcpy(h->ss_off.get(), off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(h, hipMemcpy(h->ss_x.get(), x + skip * 6, total * 6 * sizeof(double), hipMemcpyHostToDevice));
  h->ss_laps = (int)npts.size();
  h->ss_total = (int)total;
  return LMPC_OK;
}

int lmpc_ss_query_batch(lmpc_handle* h, int32_t batch, const double* query, double* ss_x, double* ss_j,
                        int32_t* n_found) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (batch < 0 || !query || !ss_x || !ss_j || !n_found)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_ss_query_batch: null pointer or negative batch");
  return ss_query_batch(h, batch, query, ss_x, ss_j, n_found, nullptr);
}

int lmpc_ss_query_idx_batch(lmpc_handle* h, int32_t batch, const double* query, int32_t* ss_idx, int32_t* n_found) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (batch < 0 || !query || !ss_idx || !n_found)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_ss_query_idx_batch: null pointer or negative batch");
  h->ss_idx_gen = h->ss_gen;
  return ss_query_batch(h, batch, query, nullptr, nullptr, n_found, ss_idx);
}

int lmpc_ss_query_host(lmpc_handle* h, const double* query, double* ss_x, double* ss_j, int32_t* n_found, double* j0) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!query || !ss_x || !ss_j || !n_found) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_ss_query_host: null pointer");
  const int rc = ss_query_check(h, LMPC_ERR_UNSUPPORTED, "");
  if (rc != LMPC_OK) return rc;
  const int S = h->cfg.num_ss_pts;
  size_t lds = 0;
  const int rl = ss_query_lds(h, &lds);
  if (rl != LMPC_OK) return rl;
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t nd = 2 + 7 * (size_t)S + 1;  // query | ss_x [6][S] | ss_j [S] | j0
  double* const d = h->ssq_dev.get();  // handle-owned staging (lmpc_create): nothing is allocated or freed per call
  int* const di = h->ssq_int.get();
  double* const host = h->ssq_host.get();
  int* const hi = h->ssq_int_host.get();
  if (!d || !di || !host) return fail(h, LMPC_ERR_RUNTIME, "lmpc_ss_query_host: staging not allocated");
  for (size_t e = 0; e < nd; ++e) host[e] = 0.0;
  host[0] = query[0];
  host[1] = query[1];
  *hi = 0;
  HIP_TRY(h, hipMemcpyAsync(d, host, nd * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(di, hi, sizeof(int), hipMemcpyHostToDevice, h->stream));
  const int rq = ss_query_launch(h, 1, d, d + 2, d + 2 + 6 * (size_t)S, di, d + 2 + 7 * (size_t)S, nullptr, lds);
  if (rq != LMPC_OK) return rq;
  HIP_TRY(h, hipMemcpyAsync(host, d, nd * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipMemcpyAsync(hi, di, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  const int nf = *hi;
  for (int j = 0; j < S; ++j) {
    for (int k = 0; k < 6; ++k) ss_x[(size_t)j * 6 + k] = host[2 + (size_t)k * S + j];  // -> column-major 6 x S
    ss_j[j] = host[2 + 6 * (size_t)S + j];
  }
  *n_found = nf;
  if (j0) *j0 = host[2 + 7 * (size_t)S];
  return LMPC_OK;
}

int lmpc_set_regression_laps(lmpc_handle* h, int32_t n_laps, const int32_t* n_pts, const double* x, const double* u,
                             const double* k, const double* t, const lmpc_regression_spec* spec) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (h->dtrack_model && n_laps != 0 && spec) return fail(h, LMPC_ERR_UNSUPPORTED, std::string("lmpc_set_regression_laps") + ": the double-track controller model is on (lmpc_dtrack_set_controller_model): the regression holds residuals against the single-track model");
  if (h->cars_model && n_laps != 0 && spec) return fail(h, LMPC_ERR_UNSUPPORTED, std::string("lmpc_set_regression_laps") + ": the per-car controller model is on (lmpc_cars_set_controller_model): the regression holds residuals against the handle's vehicle");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  reg_off(h);
  if (n_laps == 0 || !spec) return LMPC_OK;
  if (h->freg_on)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_set_regression_laps: the per-car regression is on (lmpc_fleet_ss_set_regression); switch it off first");
  if (n_laps < 0 || !n_pts || !x || !u || !k || !t) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_set_regression_laps: bad argument");
  const int nf = spec->n_in_state + spec->n_in_ctrl;
  if (!((nf == 5 && spec->n_out == 3) || (nf == 8 && spec->n_out == 6)) || spec->n_in_state < 1 || spec->n_in_state > 6 ||
      spec->n_in_ctrl < 0 || spec->n_in_ctrl > 2)
    return fail(h, LMPC_ERR_UNSUPPORTED, "regression built for (features, rows) = (5, 3) and (8, 6)");
  if (!(spec->dist_max > 0.0)) return fail(h, LMPC_ERR_ARGUMENT, "dist_max must be positive");
  for (int i = 0; i < spec->n_out; ++i)
    if (spec->out[i] < 0 || spec->out[i] > 5) return fail(h, LMPC_ERR_ARGUMENT, "regressed row out of range");
  for (int i = 0; i < spec->n_in_state; ++i)
    if (spec->in_state[i] < 0 || spec->in_state[i] > 5) return fail(h, LMPC_ERR_ARGUMENT, "feature state out of range");
  for (int i = 0; i < spec->n_in_ctrl; ++i)
    if (spec->in_ctrl[i] < 0 || spec->in_ctrl[i] > 1) return fail(h, LMPC_ERR_ARGUMENT, "feature control out of range");
  std::vector<int> valid;
  if (const int rc = reg_upload_laps(h, "lmpc_set_regression_laps", n_laps, n_pts, x, u, k, t, spec->as_written != 0, valid)) {
    reg_off(h);
    return rc;
  }
  const size_t total = (size_t)h->reg_total;
  dev_buf<int> dvalid;
  {  // dense table of the samples that have a successor (what the per-solve kernel streams)
    const int nvalid = (int)valid.size(), npad = (nvalid + 3) / 4 * 4;
    HIP_TRY(h, dvalid.alloc((size_t)nvalid));
    HIP_TRY(h, h->reg_tab.alloc((size_t)npad * (size_t)(nf + spec->n_out + 1)));
    HIP_TRY(h, hipMemcpy(dvalid.get(), valid.data(), (size_t)nvalid * sizeof(int), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(lmpc_reg_pack_kernel, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, h->stream, *spec, nvalid, npad, dvalid.get(),
                       h->reg_x.get(), h->reg_u.get(), h->reg_y.get(), h->reg_tab.get(),
                       h->reg_tab.get() + (size_t)npad * (size_t)(nf + spec->n_out));
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->reg_npad = npad;
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  // The per-solve kernel screens samples with d^2 = |q|^2 + |z|^2 - 2 z.q, whose rounding error is a few ulp of |z|^2 (a query
  // within the bandwidth has |q| <= |z| + h).  Where the largest |z|^2 exceeds 256 h^2 that error reaches 1e-13 of a weight and
  // the kernel recomputes the weights of the samples it keeps from sum (z - q)^2 (the abscissa of the IAC track, s up to 2849 m:
  // 1e-8 otherwise).  The bench's BARC features (vx, vy, w, u) stay below it and keep the cheaper loop.
  double zmax2 = 0.0;
  for (size_t j = 0; j < total; ++j) {
    double s = 0.0;
    for (int f = 0; f < spec->n_in_state; ++f) s += x[j * 6 + spec->in_state[f]] * x[j * 6 + spec->in_state[f]];
    for (int f = 0; f < spec->n_in_ctrl; ++f) s += u[j * 2 + spec->in_ctrl[f]] * u[j * 2 + spec->in_ctrl[f]];
    zmax2 = s > zmax2 ? s : zmax2;
  }
  h->reg_exact = !(zmax2 <= 256.0 * spec->dist_max * spec->dist_max);
  h->reg_total = (int)total;
  h->reg_spec = *spec;
  h->reg_on = true;
  return LMPC_OK;
}

// the same store with one feature list per regressed row (csrc/lmpc_reg_rows.h, csrc/lmpc_reg_rows_kernel.hip).  Everything that can
// refuse the call is looked at before the regression in effect is touched.
int lmpc_set_regression_laps_rows(lmpc_handle* h, int32_t n_laps, const int32_t* n_pts, const double* x, const double* u,
                                  const double* k, const double* t, const lmpc_regression_rows_spec* spec) {
  if (!h) return LMPC_ERR_ARGUMENT;
  HIP_TRY(h, hipSetDevice(h->device));
  if (n_laps == 0 || !spec) {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    reg_off(h);
    return LMPC_OK;
  }
  if (h->dtrack_model) return fail(h, LMPC_ERR_UNSUPPORTED, std::string("lmpc_set_regression_laps_rows") + ": the double-track controller model is on (lmpc_dtrack_set_controller_model): the regression holds residuals against the single-track model");
  if (h->cars_model) return fail(h, LMPC_ERR_UNSUPPORTED, std::string("lmpc_set_regression_laps_rows") + ": the per-car controller model is on (lmpc_cars_set_controller_model): the regression holds residuals against the handle's vehicle");
  if (h->freg_on)
    return fail(h, LMPC_ERR_ARGUMENT,
                "lmpc_set_regression_laps_rows: the per-car regression is on (lmpc_fleet_ss_set_regression / _rows); switch it off first");
  if (n_laps < 0 || !n_pts || !x || !u || !k || !t) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_set_regression_laps_rows: bad argument");
  lmpc_reg_rows_dev rs;
  const char* msg = nullptr;
  if (const int rc = lmpc_reg_rows_digest(spec, &rs, &msg)) return fail(h, rc, std::string("lmpc_set_regression_laps_rows: ") + msg);
  for (int l = 0; l < n_laps; ++l)
    if (n_pts[l] < 2) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_set_regression_laps_rows: a lap needs two samples");
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  reg_off(h);
  std::vector<int> valid;
  int rc = reg_upload_laps(h, "lmpc_set_regression_laps_rows", n_laps, n_pts, x, u, k, t, rs.as_written != 0, valid);
  if (rc == LMPC_OK) rc = [&]() -> int {  // dense table of the samples that have a successor, in the per-row layout
    const int nvalid = (int)valid.size(), npad = (nvalid + 3) / 4 * 4;
    dev_buf<int> dvalid;
    HIP_TRY(h, dvalid.alloc((size_t)nvalid));
    HIP_TRY(h, h->reg_tab.alloc((size_t)npad * (size_t)lmpc_reg_rows_stride(rs)));
    HIP_TRY(h, hipMemcpy(dvalid.get(), valid.data(), (size_t)nvalid * sizeof(int), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(lmpc_reg_rows_pack_kernel, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, h->stream, rs, nvalid, npad, dvalid.get(),
                       h->reg_x.get(), h->reg_u.get(), h->reg_y.get(), h->reg_tab.get());
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->reg_npad = npad;
    return LMPC_OK;
  }();
  if (rc != LMPC_OK) {
    reg_off(h);
    return rc;
  }
  h->reg_rspec = rs;
  h->reg_rows = true;
  h->reg_on = true;
  return LMPC_OK;
}

int lmpc_set_output_layout(lmpc_handle* h, int32_t layout) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (layout != LMPC_LAYOUT_SOA && layout != LMPC_LAYOUT_AOS) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_set_output_layout: unknown layout");
  h->out_aos = layout == LMPC_LAYOUT_AOS;
  return LMPC_OK;
}

int lmpc_set_warm_rounds(lmpc_handle* h, int32_t rounds) {
  if (!h) return LMPC_ERR_ARGUMENT;
  static_assert(LMPC_WARM_ROUNDS_MAX == 4, "the message below");
  if (rounds < 0 || rounds > LMPC_WARM_ROUNDS_MAX) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_set_warm_rounds: 0 (the default) or 1 .. 4 rounds");
  h->warm_rounds = rounds;
  return LMPC_OK;
}

int lmpc_set_launch_order(lmpc_handle* h, const int32_t* order, int32_t batch) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (order && batch <= 0) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_set_launch_order: an order needs its length (batch > 0)");
  h->order = order;
  h->order_n = order ? batch : 0;
  return LMPC_OK;
}

int lmpc_launch_order_from_iters(lmpc_handle* h, int32_t batch, const int32_t* iters, int32_t* order) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (batch < 0 || !iters || !order) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_launch_order_from_iters: null pointer or negative batch");
  if (batch == 0) return LMPC_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(lmpc_launch_order_kernel, dim3(1), dim3(1024), 0, h->stream, batch, iters, order);
  HIP_TRY(h, hipGetLastError());
  return LMPC_OK;
}

int lmpc_regress_batch(lmpc_handle* h, int32_t batch, const double* X_ref, const double* U_ref, double* A, double* Bm,
                       double* g) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (batch < 0 || !X_ref || !U_ref || !A || !Bm || !g)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_regress_batch: null pointer or negative batch");
  if (!h->reg_on) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_regress_batch: no regression laps set");
  if (batch == 0) return LMPC_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  return launch_regress<false>(h, batch, X_ref, U_ref, A, Bm, g);
}


// ---- fleet safe set: one recorder and one ring of laps per car (csrc/lmpc_fleet_ss.h, csrc/lmpc_fleet_ss_kernel.hip) ----
int lmpc_fleet_ss_destroy(lmpc_handle* h) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!h->fleet.B) return LMPC_OK;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  fleet_reg_off(h);  // its table is sized by this store
  h->fleet_key.release();
  h->fleet_xr.release();
  h->fleet_aux.release();
  h->fleet_meta.release();
  h->fleet_metad.release();
  h->fleet = lmpc_fleet_store{};
  h->fleet_meta_n = h->fleet_metad_n = 0;
  h->fleet_bytes = 0;
  h->fleet_L = 0.0;
  return LMPC_OK;
}

int lmpc_fleet_ss_reset(lmpc_handle* h) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!h->fleet.B) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_fleet_ss_reset: no fleet store (lmpc_fleet_ss_create)");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemsetAsync(h->fleet_meta.get(), 0, h->fleet_meta_n * sizeof(int), h->stream));
  HIP_TRY(h, hipMemsetAsync(h->fleet_metad.get(), 0, h->fleet_metad_n * sizeof(double), h->stream));
  return fleet_reg_invalidate(h);  // lap_count starts again at 0: a stamp must not meet it
}

int lmpc_fleet_ss_create(lmpc_handle* h, int32_t batch, int32_t max_pts_per_lap) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (batch < 1 || max_pts_per_lap < 1) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_fleet_ss_create: batch and max_pts_per_lap must be positive");
  if (h->cfg.max_lap_stored < 1)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_fleet_ss_create: lmpc_config.max_lap_stored must be positive (a fleet ring is bounded)");
  // 80 bytes per sample; the sample count is held below 2^36 (5.5 TB) so that no size below can overflow
  const unsigned long long slots = (unsigned long long)batch * ((unsigned long long)h->cfg.max_lap_stored + 1ull);
  if (slots > (1ull << 36) / (unsigned long long)max_pts_per_lap)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_fleet_ss_create: batch x (max_lap_stored + 1) x max_pts_per_lap is too large");
  const size_t rows = (size_t)slots * (size_t)max_pts_per_lap;
  const int rc0 = lmpc_fleet_ss_destroy(h);
  if (rc0 != LMPC_OK) return rc0;
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t Bz = (size_t)batch, meta_n = (size_t)slots + 7 * Bz, metad_n = Bz * (1 + LMPC_FLEET_DUR);
  // into local owners: a refused allocation leaves the handle without a store, and nothing behind
  dev_buf<double2> key;
  dev_buf<double> xr, aux, metad_buf;
  dev_buf<int> meta_buf;
  HIP_TRY_AS(h, "lmpc_fleet_ss_create", key.alloc(rows));
  HIP_TRY_AS(h, "lmpc_fleet_ss_create", xr.alloc(rows * 4));
  HIP_TRY_AS(h, "lmpc_fleet_ss_create", aux.alloc(rows * 4));
  HIP_TRY_AS(h, "lmpc_fleet_ss_create", meta_buf.alloc(meta_n));
  HIP_TRY_AS(h, "lmpc_fleet_ss_create", metad_buf.alloc(metad_n));
  HIP_TRY_AS(h, "lmpc_fleet_ss_create", hipMemsetAsync(meta_buf.get(), 0, meta_n * sizeof(int), h->stream));
  HIP_TRY_AS(h, "lmpc_fleet_ss_create", hipMemsetAsync(metad_buf.get(), 0, metad_n * sizeof(double), h->stream));
  int* const meta = meta_buf.get();
  double* const metad = metad_buf.get();
  lmpc_fleet_store st{};
  st.B = batch;
  st.R = h->cfg.max_lap_stored;
  st.C = max_pts_per_lap;
  st.key = key.get();
  st.xr = xr.get();
  st.aux = aux.get();
  st.npts = meta;
  st.head = meta + slots;
  st.cnt = st.head + Bz;
  st.open_n = st.cnt + Bz;
  st.flags = st.open_n + Bz;
  st.lap_count = st.flags + Bz;
  st.n_dropped = st.lap_count + Bz;
  st.dur_n = st.n_dropped + Bz;
  st.s_prev = metad;
  st.dur = metad + Bz;
  h->fleet = st;
  h->fleet_key = std::move(key);
  h->fleet_xr = std::move(xr);
  h->fleet_aux = std::move(aux);
  h->fleet_meta = std::move(meta_buf);
  h->fleet_metad = std::move(metad_buf);
  h->fleet_meta_n = meta_n;
  h->fleet_metad_n = metad_n;
  h->fleet_bytes = (int64_t)(rows * 80 + meta_n * sizeof(int) + metad_n * sizeof(double));
  h->fleet_L = 0.0;
  return LMPC_OK;
}

int lmpc_fleet_ss_bytes(const lmpc_handle* h, int64_t* bytes) {
  if (!h || !bytes) return LMPC_ERR_ARGUMENT;
  *bytes = h->fleet_bytes + h->freg_bytes;
  return LMPC_OK;
}

int lmpc_fleet_ss_record_batch(lmpc_handle* h, int32_t batch, const double* x, const double* u, const double* k, double t,
                               double total_length, const int32_t* active) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!x || !u || !k || !(total_length > 0.0)) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_fleet_ss_record_batch: null pointer or bad total_length");
  const int rc = fleet_check(h, batch, "lmpc_fleet_ss_record_batch");
  if (rc != LMPC_OK) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  h->fleet_L = total_length;
  hipLaunchKernelGGL(lmpc_fleet_ss_record_kernel, dim3((batch + 255) / 256), dim3(256), 0, h->stream, h->fleet, x, u, k, t, total_length,
                     active);
  HIP_TRY(h, hipGetLastError());
  return LMPC_OK;
}

int lmpc_fleet_ss_query_batch(lmpc_handle* h, int32_t batch, const double* query, double* ss_x, double* ss_j, int32_t* n_found) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!query || !ss_x || !ss_j || !n_found) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_fleet_ss_query_batch: null pointer");
  int rc = fleet_check(h, batch, "lmpc_fleet_ss_query_batch");
  if (rc == LMPC_OK) rc = ss_query_check(h, LMPC_ERR_ARGUMENT, "lmpc_fleet_ss_query_batch: ");
  if (rc != LMPC_OK) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(lmpc_fleet_ss_query_kernel, dim3(8 * ((batch + 7) / 8)), dim3(64), 0, h->stream, h->fleet, h->cfg.num_ss_pts,
                     h->cfg.num_ss_pts_per_lap, h->fleet_L, query, ss_x, ss_j, n_found);
  HIP_TRY(h, hipGetLastError());
  return LMPC_OK;
}

int lmpc_fleet_ss_stats(lmpc_handle* h, int32_t batch, int32_t* laps_in_ring, int32_t* lap_count, int32_t* n_dropped,
                        double* last_lap_time) {
  if (!h) return LMPC_ERR_ARGUMENT;
  const int rc = fleet_check(h, batch, "lmpc_fleet_ss_stats");
  if (rc != LMPC_OK) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(lmpc_fleet_ss_stats_kernel, dim3((batch + 255) / 256), dim3(256), 0, h->stream, h->fleet, laps_in_ring, lap_count,
                     n_dropped, last_lap_time);
  HIP_TRY(h, hipGetLastError());
  return LMPC_OK;
}

// ---- everything between two solves of a fleet LMPC period (csrc/lmpc_fleet_loop_kernel.hip) ----
// Both entry points: the validation, the constants and the launch.  dtrack: step 2's plant is the handle's double-track table
// (lmpc_fleet_loop_advance_dtrack_batch, include/lmpc_hip_fleet_dtrack.h); else the call as it always was, table or no table.
static int fleet_loop_advance(lmpc_handle* h, int32_t batch, const lmpc_track* track, const lmpc_fleet_loop* io, bool dtrack, double* gamma_y,
                              const char* who) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!io) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": io is NULL");
  const int rc = fleet_check(h, batch, who);
  if (rc != LMPC_OK) return rc;
  if (!track_ok(track)) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": bad track");
  if (!io->x || !io->u_prev || !io->X_ref || !io->U_ref || !io->T_ref || !io->bound_left || !io->bound_right || !io->curvatures ||
      !io->vel_ref || !io->phase || !io->n_learn || !io->lap_time || !io->lap_kind || !io->counters || !io->x_ic || !io->query)
    return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": a required pointer is NULL");
  const int n_trk = (io->X_trk != nullptr) + (io->U_trk != nullptr) + (io->status_trk != nullptr);
  const int n_lrn = (io->X_lrn != nullptr) + (io->U_lrn != nullptr) + (io->status_lrn != nullptr);
  if ((n_trk != 0 && n_trk != 3) || (n_lrn != 0 && n_lrn != 3))
    return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": a solution is X, U and status, or none of them");
  if (!(io->dt > 0.0) || !(io->dt_sim > 0.0) || io->n_sub < 1) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": dt, dt_sim must be positive and n_sub >= 1");
  if (io->warm_laps < 1 || io->learn_laps < 1 || io->n_rec < 1)
    return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": warm_laps, learn_laps and n_rec must be >= 1");
  if (io->plant && io->plant->model_id != LMPC_MODEL_SINGLE_TRACK_PLANAR)
    return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": plant: only single_track_planar_model is built");
  if (io->plant && io->plant->integrator != LMPC_INTEGRATOR_RK4 && io->plant->integrator != LMPC_INTEGRATOR_EULER)
    return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": plant: integrator must be LMPC_INTEGRATOR_RK4 or LMPC_INTEGRATOR_EULER");
  if ((io->X_trk && (io->X_ref == io->X_trk || io->U_ref == io->U_trk)) || (io->X_lrn && (io->X_ref == io->X_lrn || io->U_ref == io->U_lrn)))
    return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": the references must not alias a solution");
  if (dtrack) {  // one source for the plant: the double-track table, of the store's batch
    if (!h->dtrack_B) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": no double-track table (lmpc_dtrack_set_vehicles)");
    if (h->dtrack_B != batch)
      return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": the double-track table holds " + std::to_string(h->dtrack_B) + " vehicles, the store " + std::to_string(batch) + " cars");
    if (io->plant) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": plant must be NULL: the double-track table is the plant, one source for it");
    if (h->cars_B)
      return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": a car table is set (lmpc_cars_set_vehicles) beside the double-track table: one source for the plant");
  }
  if (h->cars_B && io->plant)
    return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": plant must be NULL while a car table is set (lmpc_cars_set_vehicles): one source for the plant");
  if (h->cars_B && h->cars_B != batch)
    return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": the car table holds " + std::to_string(h->cars_B) + " vehicles, the store " + std::to_string(batch) + " cars");
  if (h->out_aos) return fail(h, LMPC_ERR_UNSUPPORTED, std::string(who) + " reads the solutions in the [component][knot][batch] layout");
  HIP_TRY(h, hipSetDevice(h->device));
  lmpc_fleet_loop_consts K{};
  K.N = h->P.N;
  for (int k = 0; k < 6; ++k) K.x_min[k] = h->P.x_min[k], K.x_max[k] = h->P.x_max[k];
  K.veh = h->P.veh;
  K.plant = io->plant ? *io->plant : h->P.veh;
  lmpc_fleet_loop dev = *io;
  dev.plant = nullptr;  // (a host pointer: the kernel takes the vehicle by value)
  dev.restart_failed = io->restart_failed ? 1 : 0;
  h->fleet_L = track->L;  // what the query unrolls the laps by, as lmpc_fleet_ss_record_batch notes it
  const dim3 grid((batch + 63) / 64), block(64 * lmpc_loop_waves);
  if (dtrack) {  // the double-track instantiation: the constants, and behind them the DEVICE double-track table and gamma_y
    lmpc_fleet_loop_consts_dt Kd{};
    static_cast<lmpc_fleet_loop_consts&>(Kd) = K;
    Kd.table = h->dtrack_tab.get();
    Kd.gamma_y = gamma_y;
    hipLaunchKernelGGL(lmpc_fleet_loop_kernel<LMPC_FLEET_PLANT_DTRACK>, grid, block, 0, h->stream, Kd, h->fleet, *track, dev);
  } else if (h->cars_B) {  // the kernel's table instantiation reads the DEVICE car table where the host's vehicle pointer was
    dev.plant = reinterpret_cast<const lmpc_vehicle*>(h->cars_tab.get());
    hipLaunchKernelGGL(lmpc_fleet_loop_kernel<LMPC_FLEET_PLANT_CARS>, grid, block, 0, h->stream, K, h->fleet, *track, dev);
  } else {
    hipLaunchKernelGGL(lmpc_fleet_loop_kernel<LMPC_FLEET_PLANT_HANDLE>, grid, block, 0, h->stream, K, h->fleet, *track, dev);
  }
  HIP_TRY(h, hipGetLastError());
  return LMPC_OK;
}

int lmpc_fleet_loop_advance_batch(lmpc_handle* h, int32_t batch, const lmpc_track* track, const lmpc_fleet_loop* io) {
  return fleet_loop_advance(h, batch, track, io, false, nullptr, "lmpc_fleet_loop_advance_batch");
}

// ---- the same period on four-wheel cars (include/lmpc_hip_fleet_dtrack.h) ----
int lmpc_fleet_loop_advance_dtrack_batch(lmpc_handle* h, int32_t batch, const lmpc_track* track, const lmpc_fleet_loop* io,
                                         double* gamma_y_or_null) {
  return fleet_loop_advance(h, batch, track, io, true, gamma_y_or_null, "lmpc_fleet_loop_advance_dtrack_batch");
}

// ---- the car table: one plant vehicle per car (include/lmpc_hip_cars.h, csrc/lmpc_cars.h, csrc/lmpc_cars_kernel.hip) ----
int lmpc_cars_set_vehicles(lmpc_handle* h, int32_t batch, const lmpc_vehicle* veh) {
  if (!h) return LMPC_ERR_ARGUMENT;
  const char* who = "lmpc_cars_set_vehicles";
  if (batch < 0) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": batch is negative");
  const bool off = !veh || batch == 0;
  for (int b = 0; !off && b < batch; ++b) {
    if (veh[b].model_id != LMPC_MODEL_SINGLE_TRACK_PLANAR)
      return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": vehicle " + std::to_string(b) + ": only single_track_planar_model is built");
    if (veh[b].integrator != LMPC_INTEGRATOR_RK4 && veh[b].integrator != LMPC_INTEGRATOR_EULER)
      return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": vehicle " + std::to_string(b) + ": integrator must be LMPC_INTEGRATOR_RK4 or LMPC_INTEGRATOR_EULER");
  }
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // nothing in flight reads the older table
  if (off) {
    h->cars_tab.release();
    h->cars_B = 0;
    h->cars_model = false;  // (no table, no controller model: include/lmpc_hip_cars_model.h)
    return LMPC_OK;
  }
  const size_t B = (size_t)batch, nd = lmpc_cars_doubles(B);
  std::vector<double> host(nd, 0.0);
  int* const integ = reinterpret_cast<int*>(host.data() + (size_t)lmpc_cars_fields * B);
  for (size_t b = 0; b < B; ++b) {
    size_t f = 0;
#define LMPC_CARS_PACK_(name) host[(f++) * B + b] = veh[b].name;
    LMPC_VEHICLE_DOUBLES(LMPC_CARS_PACK_)
#undef LMPC_CARS_PACK_
    integ[b] = veh[b].integrator;
  }
  dev_buf<double> tab;  // into a local owner: a refused allocation or copy leaves the older table in effect
  HIP_TRY_AS(h, who, tab.alloc(nd));
  HIP_TRY_AS(h, who, hipMemcpy(tab.get(), host.data(), nd * sizeof(double), hipMemcpyHostToDevice));
  h->cars_tab = std::move(tab);
  h->cars_B = batch;
  return LMPC_OK;
}

int lmpc_cars_get_vehicles(lmpc_handle* h, int32_t batch, lmpc_vehicle* veh) {
  if (!h) return LMPC_ERR_ARGUMENT;
  const char* who = "lmpc_cars_get_vehicles";
  if (!h->cars_B) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": no car table (lmpc_cars_set_vehicles)");
  if (batch != h->cars_B || !veh)
    return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": veh is NULL or batch " + std::to_string(batch) + " is not the table's " + std::to_string(h->cars_B));
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  const size_t B = (size_t)batch, nd = lmpc_cars_doubles(B);
  std::vector<double> host(nd);
  HIP_TRY_AS(h, who, hipMemcpy(host.data(), h->cars_tab.get(), nd * sizeof(double), hipMemcpyDeviceToHost));
  const int* const integ = reinterpret_cast<const int*>(host.data() + (size_t)lmpc_cars_fields * B);
  for (size_t b = 0; b < B; ++b) {
    size_t f = 0;
#define LMPC_CARS_UNPACK_(name) veh[b].name = host[(f++) * B + b];
    LMPC_VEHICLE_DOUBLES(LMPC_CARS_UNPACK_)
#undef LMPC_CARS_UNPACK_
    veh[b].model_id = LMPC_MODEL_SINGLE_TRACK_PLANAR;
    veh[b].integrator = integ[b];
  }
  return LMPC_OK;
}

int lmpc_plant_step_cars_batch(lmpc_handle* h, int32_t batch, const lmpc_track* track, double* x, const double* u, double dt_sim,
                               int32_t n_sub) {
  if (!h) return LMPC_ERR_ARGUMENT;
  const char* who = "lmpc_plant_step_cars_batch";
  if (!h->cars_B) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": no car table (lmpc_cars_set_vehicles)");
  if (batch != h->cars_B)
    return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": batch " + std::to_string(batch) + " is not the table's " + std::to_string(h->cars_B));
  if (!track_ok(track) || !x || !u || !(dt_sim > 0.0) || n_sub < 1) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": bad argument");
  HIP_TRY(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(lmpc_plant_cars_kernel, dim3((batch + 255) / 256), dim3(256), 0, h->stream, h->cars_tab.get(), batch, *track, x, u, dt_sim,
                     n_sub);
  HIP_TRY(h, hipGetLastError());
  return LMPC_OK;
}

// ---- the per-car single-track CONTROLLER model (include/lmpc_hip_cars_model.h, csrc/lmpc_cars_model.h, csrc/lmpc_cars_model_kernel.hip) ----
int lmpc_linearize_cars_batch(lmpc_handle* h, int32_t batch, const double* X_ref, const double* U_ref, const double* T_ref,
                              const double* curvatures, double* A, double* Bm, double* g) {
  if (!h) return LMPC_ERR_ARGUMENT;
  const char* who = "lmpc_linearize_cars_batch";
  if (!h->cars_B) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": no car table (lmpc_cars_set_vehicles)");
  if (batch != h->cars_B)
    return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": batch " + std::to_string(batch) + " is not the table's " + std::to_string(h->cars_B));
  if (!X_ref || !U_ref || !T_ref || !curvatures || !A || !Bm || !g) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": null pointer");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, lmpc_cars_launch_linearize(h->stream, h->cars_tab.get(), h->P.N, batch, false, X_ref, U_ref, T_ref, curvatures, A, Bm, g));
  return LMPC_OK;
}

int lmpc_cars_set_controller_model(lmpc_handle* h, int32_t on) {
  if (!h) return LMPC_ERR_ARGUMENT;
  const char* who = "lmpc_cars_set_controller_model";
  if (!on) {
    h->cars_model = false;
    return LMPC_OK;
  }
  if (!h->cars_B) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": no car table (lmpc_cars_set_vehicles)");
  if (h->dtrack_model)
    return fail(h, LMPC_ERR_UNSUPPORTED, std::string(who) + ": the double-track controller model is on (lmpc_dtrack_set_controller_model): a handle solves on one model; switch it off first");
  if (h->reg_on || h->freg_on)
    return fail(h, LMPC_ERR_UNSUPPORTED, std::string(who) + ": an error-dynamics regression is in effect (" +
                                             (h->reg_on ? "lmpc_set_regression_laps / _rows" : "lmpc_fleet_ss_set_regression / _rows") +
                                             "); its residuals are against the handle's vehicle: switch it off first");
  h->cars_model = true;
  return LMPC_OK;
}

int lmpc_cars_get_controller_model(const lmpc_handle* h, int32_t* on) {
  if (!h || !on) return LMPC_ERR_ARGUMENT;
  *on = h->cars_model ? 1 : 0;
  return LMPC_OK;
}

// ---- the double-track table: one four-wheel plant vehicle per car (include/lmpc_hip_dtrack.h, csrc/lmpc_dtrack.h, csrc/lmpc_dtrack_kernel.hip) ----
int lmpc_dtrack_set_vehicles(lmpc_handle* h, int32_t batch, const lmpc_vehicle_dt* veh) {
  if (!h) return LMPC_ERR_ARGUMENT;
  const char* who = "lmpc_dtrack_set_vehicles";
  if (batch < 0) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": batch is negative");
  const bool off = !veh || batch == 0;
  for (int b = 0; !off && b < batch; ++b) {
    const std::string car = std::string(who) + ": vehicle " + std::to_string(b);
    if (veh[b].base.model_id != LMPC_MODEL_DOUBLE_TRACK_PLANAR)
      return fail(h, LMPC_ERR_ARGUMENT, car + ": model_id must be LMPC_MODEL_DOUBLE_TRACK_PLANAR");
    if (veh[b].base.integrator != LMPC_INTEGRATOR_RK4 && veh[b].base.integrator != LMPC_INTEGRATOR_EULER)
      return fail(h, LMPC_ERR_ARGUMENT, car + ": integrator must be LMPC_INTEGRATOR_RK4 or LMPC_INTEGRATOR_EULER");
    if (!(veh[b].tw_f + veh[b].tw_r > 0.0)) return fail(h, LMPC_ERR_ARGUMENT, car + ": tw_f + tw_r must be positive");
    if (veh[b].Fz0_f == 0.0 || veh[b].Fz0_r == 0.0) return fail(h, LMPC_ERR_ARGUMENT, car + ": Fz0_f and Fz0_r must not be 0");
  }
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // nothing in flight reads the older table
  if (off) {
    h->dtrack_tab.release();
    h->dtrack_B = 0;
    h->dtrack_model = false;  // (no table, no controller model: include/lmpc_hip_dtrack_model.h)
    return LMPC_OK;
  }
  const size_t nd = lmpc_dtrack_doubles((size_t)batch);
  std::vector<double> host(nd, 0.0);
  lmpc_dtrack_pack(veh, (size_t)batch, host.data());
  dev_buf<double> tab;  // into a local owner: a refused allocation or copy leaves the older table in effect
  HIP_TRY_AS(h, who, tab.alloc(nd));
  HIP_TRY_AS(h, who, hipMemcpy(tab.get(), host.data(), nd * sizeof(double), hipMemcpyHostToDevice));
  h->dtrack_tab = std::move(tab);
  h->dtrack_B = batch;
  return LMPC_OK;
}

int lmpc_dtrack_get_vehicles(lmpc_handle* h, int32_t batch, lmpc_vehicle_dt* veh) {
  if (!h) return LMPC_ERR_ARGUMENT;
  const char* who = "lmpc_dtrack_get_vehicles";
  if (!h->dtrack_B) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": no double-track table (lmpc_dtrack_set_vehicles)");
  if (batch != h->dtrack_B || !veh)
    return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": veh is NULL or batch " + std::to_string(batch) + " is not the table's " + std::to_string(h->dtrack_B));
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  const size_t nd = lmpc_dtrack_doubles((size_t)batch);
  std::vector<double> host(nd);
  HIP_TRY_AS(h, who, hipMemcpy(host.data(), h->dtrack_tab.get(), nd * sizeof(double), hipMemcpyDeviceToHost));
  lmpc_dtrack_unpack(host.data(), (size_t)batch, veh);
  return LMPC_OK;
}

int lmpc_plant_step_dtrack_batch(lmpc_handle* h, int32_t batch, const lmpc_track* track, double* x, const double* u, double dt_sim,
                                 int32_t n_sub, double* gamma_y_or_null) {
  if (!h) return LMPC_ERR_ARGUMENT;
  const char* who = "lmpc_plant_step_dtrack_batch";
  if (!h->dtrack_B) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": no double-track table (lmpc_dtrack_set_vehicles)");
  if (batch != h->dtrack_B)
    return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": batch " + std::to_string(batch) + " is not the table's " + std::to_string(h->dtrack_B));
  if (!track_ok(track) || !x || !u || !(dt_sim > 0.0) || n_sub < 1) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": bad argument");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, lmpc_dtrack_launch_step(h->stream, h->dtrack_tab.get(), batch, *track, x, u, dt_sim, n_sub, gamma_y_or_null));
  return LMPC_OK;
}

// ---- the double-track CONTROLLER model (include/lmpc_hip_dtrack_model.h, csrc/lmpc_dtrack_model.h, csrc/lmpc_dtrack_model_kernel.hip) ----
int lmpc_linearize_dtrack_batch(lmpc_handle* h, int32_t batch, const double* X_ref, const double* U_ref, const double* T_ref,
                                const double* curvatures, double* A, double* Bm, double* g) {
  if (!h) return LMPC_ERR_ARGUMENT;
  const char* who = "lmpc_linearize_dtrack_batch";
  if (!h->dtrack_B) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": no double-track table (lmpc_dtrack_set_vehicles)");
  if (batch != h->dtrack_B)
    return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": batch " + std::to_string(batch) + " is not the table's " + std::to_string(h->dtrack_B));
  if (!X_ref || !U_ref || !T_ref || !curvatures || !A || !Bm || !g) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": null pointer");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, lmpc_dtrack_launch_linearize(h->stream, h->dtrack_tab.get(), h->P.N, batch, false, X_ref, U_ref, T_ref, curvatures, A, Bm, g));
  return LMPC_OK;
}

int lmpc_dtrack_set_controller_model(lmpc_handle* h, int32_t on) {
  if (!h) return LMPC_ERR_ARGUMENT;
  const char* who = "lmpc_dtrack_set_controller_model";
  if (!on) {
    h->dtrack_model = false;
    return LMPC_OK;
  }
  if (!h->dtrack_B) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": no double-track table (lmpc_dtrack_set_vehicles)");
  if (h->cars_model)
    return fail(h, LMPC_ERR_UNSUPPORTED, std::string(who) + ": the per-car controller model is on (lmpc_cars_set_controller_model): a handle solves on one model; switch it off first");
  if (h->reg_on || h->freg_on)
    return fail(h, LMPC_ERR_UNSUPPORTED, std::string(who) + ": an error-dynamics regression is in effect (" +
                                             (h->reg_on ? "lmpc_set_regression_laps / _rows" : "lmpc_fleet_ss_set_regression / _rows") +
                                             "); its residuals are against the single-track model: switch it off first");
  h->dtrack_model = true;
  return LMPC_OK;
}

int lmpc_dtrack_get_controller_model(const lmpc_handle* h, int32_t* on) {
  if (!h || !on) return LMPC_ERR_ARGUMENT;
  *on = h->dtrack_model ? 1 : 0;
  return LMPC_OK;
}

int lmpc_fleet_ss_load(lmpc_handle* h, int32_t car, int32_t n_laps, const int32_t* n_pts, const double* x, const double* u,
                       const double* k, const double* t, double total_length) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!h->fleet.B) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_fleet_ss_load: no fleet store (lmpc_fleet_ss_create)");
  if (car < -1 || car >= h->fleet.B || n_laps < 0 || (n_laps > 0 && (!n_pts || !x || !u || !k || !t)) || !(total_length > 0.0))
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_fleet_ss_load: bad argument");
  for (int l = 0; l < n_laps; ++l) {
    if (n_pts[l] < 1) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_fleet_ss_load: empty lap");
    if (n_pts[l] > h->fleet.C)
      return fail(h, LMPC_ERR_ARGUMENT, "lmpc_fleet_ss_load: lap " + std::to_string(l) + " has " + std::to_string(n_pts[l]) +
                                            " samples, the store's capacity is " + std::to_string(h->fleet.C));
  }
  h->fleet_L = total_length;
  if (n_laps == 0) return LMPC_OK;
  // the ring keeps the last max_lap_stored laps: the earlier ones of a longer list would be pushed out again (their count stays)
  const int first = n_laps > h->fleet.R ? n_laps - h->fleet.R : 0;
  std::vector<int> ln, lo;
  size_t skip = 0, kept = 0;
  for (int l = 0; l < n_laps; ++l) {
    if (l < first) {
      skip += (size_t)n_pts[l];
      continue;
    }
    lo.push_back((int)kept);
    ln.push_back(n_pts[l]);
    kept += (size_t)n_pts[l];
  }
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  const int nl = (int)ln.size();
  dev_buf<double> dev;  // upload-time temporaries
  dev_buf<int> devi_buf;
#define LOAD_TRY(expr) HIP_TRY_AS(h, "lmpc_fleet_ss_load", expr)
  LOAD_TRY(dev.alloc(kept * 10));
  LOAD_TRY(devi_buf.alloc((size_t)2 * nl));
  double *dx = dev.get(), *du = dx + kept * 6, *dk = dx + kept * 8, *dt = dx + kept * 9;
  int* devi = devi_buf.get();
  LOAD_TRY(hipMemcpy(dx, x + skip * 6, kept * 6 * sizeof(double), hipMemcpyHostToDevice));
  LOAD_TRY(hipMemcpy(du, u + skip * 2, kept * 2 * sizeof(double), hipMemcpyHostToDevice));
  LOAD_TRY(hipMemcpy(dk, k + skip, kept * sizeof(double), hipMemcpyHostToDevice));
  LOAD_TRY(hipMemcpy(dt, t + skip, kept * sizeof(double), hipMemcpyHostToDevice));
  LOAD_TRY(hipMemcpy(devi, ln.data(), (size_t)nl * sizeof(int), hipMemcpyHostToDevice));
  LOAD_TRY(hipMemcpy(devi + nl, lo.data(), (size_t)nl * sizeof(int), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(lmpc_fleet_ss_load_kernel, dim3(car < 0 ? h->fleet.B : 1), dim3(256), 0, h->stream, h->fleet, (int)car, nl, devi,
                     devi + nl, dx, du, dk, dt);
  LOAD_TRY(hipGetLastError());
  if (const int rc = fleet_reg_invalidate(h)) return rc;
  LOAD_TRY(hipStreamSynchronize(h->stream));
  if (first > 0) {  // SafeSetRecorder::load counts every lap it adds (safe_set.cpp:270)
    // (the laps that did not fit the ring were added and pushed out again upstream: they count)
    std::vector<int> lc((size_t)h->fleet.B);
    LOAD_TRY(hipMemcpy(lc.data(), h->fleet.lap_count, lc.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int b = 0; b < h->fleet.B; ++b)
      if (car < 0 || b == car) lc[(size_t)b] += first;
    LOAD_TRY(hipMemcpy(h->fleet.lap_count, lc.data(), lc.size() * sizeof(int), hipMemcpyHostToDevice));
  }
#undef LOAD_TRY
  return LMPC_OK;
}

int lmpc_fleet_ss_get_laps(lmpc_handle* h, int32_t car, int32_t* n_laps, int32_t* n_pts, double* x, double* u, double* k, double* t) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!h->fleet.B) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_fleet_ss_get_laps: no fleet store (lmpc_fleet_ss_create)");
  if (car < 0 || car >= h->fleet.B || !n_laps) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_fleet_ss_get_laps: bad car or null n_laps");
  if ((x || u || k || t) && !n_pts) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_fleet_ss_get_laps: the sample arrays need n_pts");
  const lmpc_fleet_store& st = h->fleet;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  const int R1 = st.R + 1;
  int head = 0, cnt = 0;
  std::vector<int> np((size_t)R1);
  HIP_TRY(h, hipMemcpy(&head, st.head + car, sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(h, hipMemcpy(&cnt, st.cnt + car, sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(h, hipMemcpy(np.data(), st.npts + (size_t)car * R1, (size_t)R1 * sizeof(int), hipMemcpyDeviceToHost));
  if (head < 0 || head >= R1 || cnt < 0 || cnt > st.R) return fail(h, LMPC_ERR_RUNTIME, "lmpc_fleet_ss_get_laps: corrupt ring state");
  *n_laps = cnt;
  std::vector<double> key, xr, ax;
  size_t o = 0;
  for (int a = 0; a < cnt; ++a) {  // oldest first
    const int sl = ((head - cnt + a) % R1 + R1) % R1;
    const int n = np[(size_t)sl] < st.C ? np[(size_t)sl] : st.C;
    if (n_pts) n_pts[a] = n;
    if (!(x || u || k || t) || n < 1) continue;
    const size_t row = ((size_t)car * R1 + sl) * st.C;
    key.resize((size_t)n * 2);
    xr.resize((size_t)n * 4);
    ax.resize((size_t)n * 4);
    HIP_TRY(h, hipMemcpy(key.data(), st.key + row, (size_t)n * 16, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(xr.data(), st.xr + row * 4, (size_t)n * 32, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(ax.data(), st.aux + row * 4, (size_t)n * 32, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i, ++o) {
      if (x) {
        x[o * 6] = key[(size_t)i * 2];
        x[o * 6 + 1] = key[(size_t)i * 2 + 1];
        for (int c = 0; c < 4; ++c) x[o * 6 + 2 + c] = xr[(size_t)i * 4 + c];
      }
      if (u) {
        u[o * 2] = ax[(size_t)i * 4];
        u[o * 2 + 1] = ax[(size_t)i * 4 + 1];
      }
      if (k) k[o] = ax[(size_t)i * 4 + 2];
      if (t) t[o] = ax[(size_t)i * 4 + 3];
    }
  }
  return LMPC_OK;
}

// ---- per-car error-dynamics regression on the fleet store (csrc/lmpc_fleet_reg.h, csrc/lmpc_fleet_reg_kernel.hip) ----
int lmpc_fleet_ss_set_regression(lmpc_handle* h, const lmpc_regression_spec* spec) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!spec) {
    (void)hipSetDevice(h->device);
    fleet_reg_off(h);
    return LMPC_OK;
  }
  if (h->dtrack_model) return fail(h, LMPC_ERR_UNSUPPORTED, std::string("lmpc_fleet_ss_set_regression") + ": the double-track controller model is on (lmpc_dtrack_set_controller_model): the regression holds residuals against the single-track model");
  if (h->cars_model) return fail(h, LMPC_ERR_UNSUPPORTED, std::string("lmpc_fleet_ss_set_regression") + ": the per-car controller model is on (lmpc_cars_set_controller_model): the regression holds residuals against the handle's vehicle");
  if (!h->fleet.B) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_fleet_ss_set_regression: no fleet store (lmpc_fleet_ss_create)");
  if (h->reg_on)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_fleet_ss_set_regression: lmpc_set_regression_laps is in effect; switch it off first");
  const int nf = spec->n_in_state + spec->n_in_ctrl;
  if (!((nf == 5 && spec->n_out == 3) || (nf == 8 && spec->n_out == 6)) || spec->n_in_state < 1 || spec->n_in_state > 6 ||
      spec->n_in_ctrl < 0 || spec->n_in_ctrl > 2)
    return fail(h, LMPC_ERR_UNSUPPORTED, "regression built for (features, rows) = (5, 3) and (8, 6)");
  if (!(spec->dist_max > 0.0)) return fail(h, LMPC_ERR_ARGUMENT, "dist_max must be positive");
  for (int i = 0; i < spec->n_out; ++i)
    if (spec->out[i] < 0 || spec->out[i] > 5) return fail(h, LMPC_ERR_ARGUMENT, "regressed row out of range");
  for (int i = 0; i < spec->n_in_state; ++i)
    if (spec->in_state[i] < 0 || spec->in_state[i] > 5) return fail(h, LMPC_ERR_ARGUMENT, "feature state out of range");
  for (int i = 0; i < spec->n_in_ctrl; ++i)
    if (spec->in_ctrl[i] < 0 || spec->in_ctrl[i] > 1) return fail(h, LMPC_ERR_ARGUMENT, "feature control out of range");
  if (const int rc = fleet_reg_table_setup(h, "lmpc_fleet_ss_set_regression", (size_t)(nf + spec->n_out + 1))) return rc;
  h->freg_spec = *spec;
  h->freg_rows = false;
  h->freg_on = true;
  return LMPC_OK;
}

// the same with one feature list per regressed row (csrc/lmpc_reg_rows.h, csrc/lmpc_fleet_reg_rows_kernel.hip)
int lmpc_fleet_ss_set_regression_rows(lmpc_handle* h, const lmpc_regression_rows_spec* spec) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!spec) {
    (void)hipSetDevice(h->device);
    fleet_reg_off(h);
    return LMPC_OK;
  }
  if (h->dtrack_model) return fail(h, LMPC_ERR_UNSUPPORTED, std::string("lmpc_fleet_ss_set_regression_rows") + ": the double-track controller model is on (lmpc_dtrack_set_controller_model): the regression holds residuals against the single-track model");
  if (h->cars_model) return fail(h, LMPC_ERR_UNSUPPORTED, std::string("lmpc_fleet_ss_set_regression_rows") + ": the per-car controller model is on (lmpc_cars_set_controller_model): the regression holds residuals against the handle's vehicle");
  if (!h->fleet.B) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_fleet_ss_set_regression_rows: no fleet store (lmpc_fleet_ss_create)");
  if (h->reg_on)
    return fail(h, LMPC_ERR_ARGUMENT,
                "lmpc_fleet_ss_set_regression_rows: lmpc_set_regression_laps / _rows is in effect; switch it off first");
  lmpc_reg_rows_dev rs;
  const char* msg = nullptr;
  if (const int rc = lmpc_reg_rows_digest(spec, &rs, &msg)) return fail(h, rc, std::string("lmpc_fleet_ss_set_regression_rows: ") + msg);
  if (const int rc = fleet_reg_table_setup(h, "lmpc_fleet_ss_set_regression_rows", (size_t)lmpc_reg_rows_stride(rs))) return rc;
  h->freg_rspec = rs;
  h->freg_rows = true;
  h->freg_on = true;
  return LMPC_OK;
}

int lmpc_fleet_ss_regress_batch(lmpc_handle* h, int32_t batch, const double* X_ref, const double* U_ref, double* A, double* Bm,
                                double* g) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!X_ref || !U_ref || !A || !Bm || !g) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_fleet_ss_regress_batch: null pointer");
  const int rc = fleet_check(h, batch, "lmpc_fleet_ss_regress_batch");
  if (rc != LMPC_OK) return rc;
  if (!h->freg_on) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_fleet_ss_regress_batch: not switched on (lmpc_fleet_ss_set_regression)");
  HIP_TRY(h, hipSetDevice(h->device));
  return launch_fleet_regress(h, false, X_ref, U_ref, A, Bm, g);
}

// ---- batched extended Kalman filter, one per car (csrc/lmpc_ekf.h, csrc/lmpc_ekf_kernel.hip) ----
int lmpc_ekf_destroy(lmpc_handle* h) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!h->ekf.B) return LMPC_OK;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  h->ekf_xup.release();
  h->ekf_K.release();
  h->ekf = lmpc_ekf_store{};
  h->ekf_obs.clear();
  h->ekf_initialized = false;
  h->ekf_ns = 0;
  return LMPC_OK;
}

int lmpc_ekf_create(lmpc_handle* h, int32_t batch, const lmpc_ekf_config* cfg) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!cfg || batch < 1 || batch > (1 << 24)) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_ekf_create: null config or batch outside 1 .. 2^24");
  const int rc0 = lmpc_ekf_destroy(h);
  if (rc0 != LMPC_OK) return rc0;
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t Bz = (size_t)batch;
  dev_buf<double> xup;  // a local owner: a refused allocation leaves the handle without a filter
  HIP_TRY_AS(h, "lmpc_ekf_create", xup.alloc(44 * Bz));
  HIP_TRY_AS(h, "lmpc_ekf_create", hipMemsetAsync(xup.get(), 0, 44 * Bz * sizeof(double), h->stream));  // u_ starts at zero (:40)
  h->ekf_xup = std::move(xup);
  h->ekf_cfg = *cfg;
  h->ekf.B = batch;
  h->ekf.nzsum = 0;
  h->ekf.x = h->ekf_xup.get();
  h->ekf.u = h->ekf.x + 6 * Bz;
  h->ekf.P = h->ekf.u + 2 * Bz;
  h->ekf.K = nullptr;
  lmpc_ekf_seed seed;
  std::memcpy(seed.x0, cfg->x0, sizeof(seed.x0));
  std::memcpy(seed.P0, cfg->P0, sizeof(seed.P0));
  HIP_TRY_AS(h, "lmpc_ekf_create", lmpc_ekf_seed_launch(h->stream, h->ekf, seed, nullptr, nullptr));
  return LMPC_OK;
}

int lmpc_ekf_register_observation(lmpc_handle* h, int32_t nz, const int32_t* rows, int32_t* obs_id) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!h->ekf.B) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_ekf_register_observation: no filter (lmpc_ekf_create)");
  if (h->ekf_initialized) return fail(h, LMPC_ERR_ARGUMENT, "Changes to observations are not allowed after the filter is initialized.");
  if (!rows || !obs_id || nz < 1 || nz > 6)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_ekf_register_observation: null pointer or nz outside 1 .. 6");
  lmpc_ekf_obs ob{};
  ob.nz = nz;
  ob.koff = h->ekf.nzsum;
  for (int a = 0; a < nz; ++a) {
    if (rows[a] < 0 || rows[a] > 5) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_ekf_register_observation: a row outside 0 .. 5");
    for (int c = 0; c < a; ++c)
      if (rows[c] == rows[a]) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_ekf_register_observation: the rows of an observation must be distinct");
    ob.rows[a] = rows[a];
  }
  // K_ grows by nz zero columns (:95-98); no update has run yet, so the whole gain is zero
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  const size_t n = 6 * (size_t)(h->ekf.nzsum + nz) * (size_t)h->ekf.B;
  dev_buf<double> K;
  HIP_TRY_AS(h, "lmpc_ekf_register_observation", K.alloc(n));
  HIP_TRY_AS(h, "lmpc_ekf_register_observation", hipMemsetAsync(K.get(), 0, n * sizeof(double), h->stream));
  h->ekf_K = std::move(K);
  h->ekf.K = h->ekf_K.get();
  h->ekf.nzsum += nz;
  *obs_id = (int32_t)h->ekf_obs.size();
  h->ekf_obs.push_back(ob);
  return LMPC_OK;
}

int lmpc_ekf_initialize(lmpc_handle* h, int64_t timestamp_ns) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!h->ekf.B) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_ekf_initialize: no filter (lmpc_ekf_create)");
  if (h->ekf_obs.empty()) return fail(h, LMPC_ERR_ARGUMENT, "No observation has been registered for the filter.");
  h->ekf_initialized = true;
  h->ekf_ns = timestamp_ns;  // x and P are not reset (:108-109 are comments)
  return LMPC_OK;
}

int lmpc_ekf_set_state(lmpc_handle* h, int32_t batch, const double* x, const double* P) {
  if (!h) return LMPC_ERR_ARGUMENT;
  const int rc = ekf_check(h, batch, "lmpc_ekf_set_state");
  if (rc != LMPC_OK) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  lmpc_ekf_seed seed;
  std::memcpy(seed.x0, h->ekf_cfg.x0, sizeof(seed.x0));
  std::memcpy(seed.P0, h->ekf_cfg.P0, sizeof(seed.P0));
  HIP_TRY(h, lmpc_ekf_seed_launch(h->stream, h->ekf, seed, x, P));
  return LMPC_OK;
}

int lmpc_ekf_update_control(lmpc_handle* h, int32_t batch, const double* u) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!u) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_ekf_update_control: null pointer");
  const int rc = ekf_check(h, batch, "lmpc_ekf_update_control");
  if (rc != LMPC_OK) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemcpyAsync(h->ekf.u, u, 2 * (size_t)batch * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  return LMPC_OK;
}

int lmpc_ekf_update_batch(lmpc_handle* h, int32_t batch, int32_t obs_id, const double* z, const double* R, int64_t timestamp_ns, double* x_out,
                          double* P_out, double* Kz_out, int32_t* flags) {
  if (!h) return LMPC_ERR_ARGUMENT;
  const int rc = ekf_check(h, batch, "lmpc_ekf_update_batch");
  if (rc != LMPC_OK) return rc;
  if (!h->ekf_initialized)
    return fail(h, LMPC_ERR_ARGUMENT, "Call EKFStateEstimator::initialize() before making any observation updates.");
  if (obs_id < -1 || obs_id >= (int32_t)h->ekf_obs.size())
    return fail(h, LMPC_ERR_ARGUMENT, "The observation name \"" + std::to_string(obs_id) + "\" is not found.");
  if (obs_id >= 0 && (!z || !R)) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_ekf_update_batch: an observation needs z and R");
  HIP_TRY(h, hipSetDevice(h->device));
  // a timestamp that jumps back only sets the time upstream; the negative dt computed before is still used (:130-146)
  const double dt = (double)(timestamp_ns - h->ekf_ns) * 1e-9;
  lmpc_ekf_consts cst;
  std::memcpy(cst.Q, h->ekf_cfg.Q, sizeof(cst.Q));
  std::memcpy(cst.x_min, h->ekf_cfg.x_min, sizeof(cst.x_min));
  std::memcpy(cst.x_max, h->ekf_cfg.x_max, sizeof(cst.x_max));
  const lmpc_ekf_out out{x_out, P_out, obs_id >= 0 ? Kz_out : nullptr, flags};
  HIP_TRY(h, lmpc_ekf_launch(h->stream, h->ekf, h->P.veh, cst, obs_id >= 0 ? &h->ekf_obs[(size_t)obs_id] : nullptr, dt, z, R, out));
  h->ekf_ns = timestamp_ns;
  return LMPC_OK;
}

int lmpc_ekf_get(lmpc_handle* h, int32_t batch, double* x, double* P, double* K, int64_t* timestamp_ns, int32_t* initialized) {
  if (!h) return LMPC_ERR_ARGUMENT;
  const int rc = ekf_check(h, batch, "lmpc_ekf_get");
  if (rc != LMPC_OK) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t Bz = (size_t)batch * sizeof(double);
  if (x) HIP_TRY(h, hipMemcpyAsync(x, h->ekf.x, 6 * Bz, hipMemcpyDeviceToDevice, h->stream));
  if (P) HIP_TRY(h, hipMemcpyAsync(P, h->ekf.P, 36 * Bz, hipMemcpyDeviceToDevice, h->stream));
  if (K && h->ekf.nzsum) HIP_TRY(h, hipMemcpyAsync(K, h->ekf.K, 6 * (size_t)h->ekf.nzsum * Bz, hipMemcpyDeviceToDevice, h->stream));
  if (timestamp_ns) *timestamp_ns = h->ekf_ns;
  if (initialized) *initialized = h->ekf_initialized ? 1 : 0;
  return LMPC_OK;
}

// ---- batched time-varying LQR, one controller per car (csrc/lmpc_lqr.h, csrc/lmpc_lqr_kernel.hip) ----
int lmpc_lqr_destroy(lmpc_handle* h) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!h->lqr.max_batch) return LMPC_OK;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  h->lqr_ws.release();
  h->lqr = lmpc_lqr_store{};
  return LMPC_OK;
}

int lmpc_lqr_create(lmpc_handle* h, int32_t max_batch, const lmpc_lqr_config* cfg) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!cfg) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_lqr_create: null config");
  if (max_batch < 1 || max_batch > (1 << 22)) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_lqr_create: max_batch outside 1 .. 2^22");
  if (cfg->N < 2 || cfg->N > 4096) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_lqr_create: N outside 2 .. 4096");
  if (!(cfg->dt > 0.0) || !std::isfinite(cfg->dt)) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_lqr_create: dt must be positive and finite");
  const int rc0 = lmpc_lqr_destroy(h);
  if (rc0 != LMPC_OK) return rc0;
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t stages = (size_t)(cfg->N - 1) * (size_t)max_batch;
  dev_buf<double> ws;  // a local owner: a refused allocation leaves the handle without a controller
  HIP_TRY_AS(h, "lmpc_lqr_create", ws.alloc(76 + 60 * stages));
  double host[76];
  std::memcpy(host, cfg->Q, sizeof(cfg->Q));
  std::memcpy(host + 36, cfg->R, sizeof(cfg->R));
  std::memcpy(host + 40, cfg->Qf, sizeof(cfg->Qf));
  HIP_TRY_AS(h, "lmpc_lqr_create", hipMemcpyAsync(ws.get(), host, sizeof(host), hipMemcpyHostToDevice, h->stream));
  HIP_TRY_AS(h, "lmpc_lqr_create", hipStreamSynchronize(h->stream));  // `host` is on this frame
  h->lqr_ws = std::move(ws);
  h->lqr.max_batch = max_batch;
  h->lqr.N = cfg->N;
  h->lqr.dt = cfg->dt;
  h->lqr.cfg = h->lqr_ws.get();
  h->lqr.AB = h->lqr.cfg + 76;
  h->lqr.K = h->lqr.AB + 48 * stages;
  return LMPC_OK;
}

int lmpc_lqr_solve_batch(lmpc_handle* h, int32_t batch, const double* x_ic, const double* X_ref, const double* U_ref, double* X_optm,
                         double* U_optm, double* K, double* P0, int32_t* flags) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!h->lqr.max_batch) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_lqr_solve_batch: no controller (lmpc_lqr_create)");
  if (batch < 1 || batch > h->lqr.max_batch)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_lqr_solve_batch: batch " + std::to_string(batch) + " outside 1 .. " + std::to_string(h->lqr.max_batch));
  if (!x_ic || !X_ref || !U_ref || !X_optm || !U_optm) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_lqr_solve_batch: null pointer");
  HIP_TRY(h, hipSetDevice(h->device));
  const lmpc_lqr_io io{x_ic, X_ref, U_ref, X_optm, U_optm, K, P0, flags};
  HIP_TRY(h, lmpc_lqr_launch(h->stream, h->lqr, h->P.veh, batch, io));
  return LMPC_OK;
}

// ---- spline track: the interpolants on the device, global <-> Frenet (lmpc_track_kernel.hip) ----

int lmpc_spline_track_create(lmpc_handle* h, double L, int32_t P, const double* breaks, const double* coef, int32_t n_wp,
                             const double* wp_x, const double* wp_y, const double* wp_s, lmpc_spline_track** track) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!track) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_spline_track_create: null track");
  *track = nullptr;
  if (!(L > 0.0) || !std::isfinite(L) || P < 1 || n_wp < 2 || !breaks || !coef || !wp_x || !wp_y || !wp_s)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_spline_track_create: null pointer, L <= 0, P < 1 or n_wp < 2");
  for (int i = 0; i <= P; ++i)
    if (!std::isfinite(breaks[i]) || (i > 0 && !(breaks[i] > breaks[i - 1])))
      return fail(h, LMPC_ERR_ARGUMENT, "lmpc_spline_track_create: breaks must be finite and strictly increasing");
  // the wrapped abscissa lies in [0, L]: the pieces have to cover it, or the end pieces would extrapolate over part of the lap
  if (breaks[0] > 0.0 || breaks[P] < L) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_spline_track_create: the breaks do not cover [0, L]");
  for (size_t e = 0; e < (size_t)5 * P * 4; ++e)
    if (!std::isfinite(coef[e])) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_spline_track_create: non-finite coefficient");
  for (int j = 0; j < n_wp; ++j)
    if (!std::isfinite(wp_x[j]) || !std::isfinite(wp_y[j]) || !std::isfinite(wp_s[j]))
      return fail(h, LMPC_ERR_ARGUMENT, "lmpc_spline_track_create: non-finite waypoint");
  // one record per piece (x | y | vel | left | right), waypoints as (x, y) pairs, the median waypoint spacing
  std::vector<double> rec((size_t)P * LMPC_TRACK_COEF), xy((size_t)n_wp * 2), gap((size_t)n_wp - 1);
  for (int c = 0; c < 5; ++c)
    for (int i = 0; i < P; ++i)
      for (int k = 0; k < 4; ++k) rec[(size_t)i * LMPC_TRACK_COEF + 4 * c + k] = coef[((size_t)c * P + i) * 4 + k];
  for (int j = 0; j < n_wp; ++j) xy[2 * (size_t)j] = wp_x[j], xy[2 * (size_t)j + 1] = wp_y[j];
  for (int j = 0; j + 1 < n_wp; ++j) gap[j] = wp_s[j + 1] - wp_s[j];
  std::sort(gap.begin(), gap.end());
  const size_t ng = gap.size();
  const double hbar = ng % 2 ? gap[ng / 2] : (gap[ng / 2 - 1] + gap[ng / 2]) / 2.0;
  if (!(hbar > 0.0)) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_spline_track_create: the waypoint abscissae must increase");
  lmpc_spline_track* t = new (std::nothrow) lmpc_spline_track();
  if (!t) return fail(h, LMPC_ERR_RUNTIME, "lmpc_spline_track_create: out of memory");
  auto upload = [&]() -> int {
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, t->breaks.alloc((size_t)P + 1));
    HIP_TRY(h, t->coef.alloc(rec.size()));
    HIP_TRY(h, t->wp_xy.alloc(xy.size()));
    HIP_TRY(h, t->wp_s.alloc((size_t)n_wp));
    HIP_TRY(h, hipMemcpyAsync(t->breaks.get(), breaks, ((size_t)P + 1) * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(t->coef.get(), rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(t->wp_xy.get(), xy.data(), xy.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(t->wp_s.get(), wp_s, (size_t)n_wp * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LMPC_OK;
  };
  const int rc = upload();
  if (rc != LMPC_OK) {
    (void)hipStreamSynchronize(h->stream);  // (a copy may still read the host vectors)
    delete t;
    return rc;
  }
  t->device = h->device;
  t->view = lmpc_spline_view{L, hbar, P, n_wp, t->breaks.get(), t->coef.get(), t->wp_xy.get(), t->wp_s.get()};
  *track = t;
  return LMPC_OK;
}

int lmpc_spline_track_destroy(lmpc_handle* h, lmpc_spline_track* track) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!track) return LMPC_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // a launch that reads the tables may still be queued
  delete track;
  return LMPC_OK;
}

}  // extern "C"

namespace {
int spline_track_check(lmpc_handle* h, const lmpc_spline_track* track, const char* who) {
  if (!track) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": null track");
  if (track->device != h->device) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": the track lives on another device");
  return LMPC_OK;
}

int track_sample(lmpc_handle* h, const lmpc_spline_track* track, int32_t n, const double* s, double* x, double* y, double* yaw,
                 double* curvature, double* left, double* right, double* vel) {
  HIP_TRY(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(lmpc_track_sample_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, track->view, n, s, x, y, yaw, curvature, left,
                     right, vel);
  HIP_TRY(h, hipGetLastError());
  return LMPC_OK;
}
}  // namespace

extern "C" {

int lmpc_track_sample_batch(lmpc_handle* h, const lmpc_spline_track* track, int32_t n, const double* s, double* out) {
  if (!h) return LMPC_ERR_ARGUMENT;
  const int rc = spline_track_check(h, track, "lmpc_track_sample_batch");
  if (rc != LMPC_OK) return rc;
  if (n < 0 || !s || !out) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_track_sample_batch: null pointer or negative n");
  if (n == 0) return LMPC_OK;
  const size_t m = (size_t)n;
  return track_sample(h, track, n, s, out, out + m, out + 2 * m, out + 3 * m, out + 4 * m, out + 5 * m, out + 6 * m);
}

int lmpc_spline_track_tabulate(lmpc_handle* h, const lmpc_spline_track* track, int32_t M, double* curvature, double* bound_left,
                               double* bound_right, double* vel) {
  if (!h) return LMPC_ERR_ARGUMENT;
  const int rc = spline_track_check(h, track, "lmpc_spline_track_tabulate");
  if (rc != LMPC_OK) return rc;
  if (M < 2 || !curvature || !bound_left || !bound_right || !vel)  // (an lmpc_track has at least two samples)
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_spline_track_tabulate: null pointer or M < 2");
  return track_sample(h, track, M, nullptr, nullptr, nullptr, nullptr, curvature, bound_left, bound_right, vel);
}

int lmpc_global_to_frenet_batch(lmpc_handle* h, const lmpc_spline_track* track, int32_t B, const double* pose, const double* s0,
                                const int32_t* seeded, double* frenet, int32_t* status) {
  if (!h) return LMPC_ERR_ARGUMENT;
  const int rc = spline_track_check(h, track, "lmpc_global_to_frenet_batch");
  if (rc != LMPC_OK) return rc;
  if (B < 0 || !pose || !frenet || !status || (seeded && !s0))
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_global_to_frenet_batch: null pointer, negative batch, or `seeded` without s0");
  if (B == 0) return LMPC_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(lmpc_track_project_kernel, dim3((B + 63) / 64), dim3(64), 0, h->stream, track->view, B, pose, s0, seeded, frenet, status);
  HIP_TRY(h, hipGetLastError());
  return LMPC_OK;
}

int lmpc_frenet_to_global_batch(lmpc_handle* h, const lmpc_spline_track* track, int32_t B, int32_t n, const double* X, double* pose) {
  if (!h) return LMPC_ERR_ARGUMENT;
  const int rc = spline_track_check(h, track, "lmpc_frenet_to_global_batch");
  if (rc != LMPC_OK) return rc;
  if (B < 0 || n < 1 || !X || !pose) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_frenet_to_global_batch: null pointer, negative batch or n < 1");
  if (B == 0) return LMPC_OK;
  const long long count = (long long)n * B;
  if (count > (1LL << 31) * 256 - 256) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_frenet_to_global_batch: n x batch too large");
  HIP_TRY(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(lmpc_track_to_global_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, track->view, count, X, pose);
  HIP_TRY(h, hipGetLastError());
  return LMPC_OK;
}

// ---- the fused estimated period (include/lmpc_hip_estimated.h, csrc/lmpc_estimated.h, csrc/lmpc_estimated_loop_kernel.hip) ----
// Every check stands in front of the launch and of the clock: a refused call has written nothing and moved nothing.
int lmpc_loop_advance_estimated_batch(lmpc_handle* h, int32_t batch, const lmpc_track* track, const lmpc_spline_track* spline,
                                      const lmpc_estimated_loop* io) {
  if (!h) return LMPC_ERR_ARGUMENT;
  const std::string who = "lmpc_loop_advance_estimated_batch";
  if (!io) return fail(h, LMPC_ERR_ARGUMENT, who + ": null io");
  int rc = ekf_check(h, batch, who.c_str());
  if (rc != LMPC_OK) return rc;
  if (!h->ekf_initialized) return fail(h, LMPC_ERR_ARGUMENT, who + ": the filter is not initialised (lmpc_ekf_initialize)");
  const int32_t n_obs = (int32_t)h->ekf_obs.size();
  if (io->obs_vel < 0 || io->obs_vel >= n_obs || io->obs_pose < 0 || io->obs_pose >= n_obs)
    return fail(h, LMPC_ERR_ARGUMENT, who + ": an observation id that was not registered");
  if (!track_ok(track)) return fail(h, LMPC_ERR_ARGUMENT, who + ": null or empty track table");
  rc = spline_track_check(h, spline, who.c_str());
  if (rc != LMPC_OK) return rc;
  if (!io->X_optm || !io->U_optm || !io->status || !io->x || !io->u_prev || !io->x_ic || !io->X_ref || !io->U_ref || !io->T_ref ||
      !io->bound_left || !io->bound_right || !io->curvatures || !io->vel_ref || !io->noise_vel || !io->R_vel || !io->noise_pose || !io->R_pose)
    return fail(h, LMPC_ERR_ARGUMENT, who + ": null required pointer");
  if (!(io->dt > 0.0) || !(io->dt_sim > 0.0)) return fail(h, LMPC_ERR_ARGUMENT, who + ": dt and dt_sim must be positive");
  if (io->n_sub < 2 || io->n_sub % 2) return fail(h, LMPC_ERR_ARGUMENT, who + ": n_sub must be even and at least 2 (the velocity observation sits at mid-period)");
  if (io->X_ref == io->X_optm || io->U_ref == io->U_optm) return fail(h, LMPC_ERR_ARGUMENT, who + ": the references must not alias the solution");
  if (h->out_aos) return fail(h, LMPC_ERR_UNSUPPORTED, who + " reads the solution in the [component][knot][batch] layout");
  if (h->cars_model || h->dtrack_model)
    return fail(h, LMPC_ERR_UNSUPPORTED, who + ": a controller-model switch is on (lmpc_cars_set_controller_model / lmpc_dtrack_set_controller_model): this call rolls out on the handle's vehicle");
  lmpc_estimated_consts K;
  K.obs_vel = h->ekf_obs[(size_t)io->obs_vel];
  K.obs_pose = h->ekf_obs[(size_t)io->obs_pose];
  bool families = K.obs_vel.nz <= 3 && K.obs_pose.nz <= 3;
  for (int a = 0; families && a < K.obs_vel.nz; ++a) families = K.obs_vel.rows[a] >= 3;
  for (int a = 0; families && a < K.obs_pose.nz; ++a) families = K.obs_pose.rows[a] <= 2;
  if (!families)
    return fail(h, LMPC_ERR_UNSUPPORTED, who + ": obs_vel must observe 1 - 3 rows within {3, 4, 5} and obs_pose 1 - 3 rows within {0, 1, 2}");
  HIP_TRY(h, hipSetDevice(h->device));
  K.veh = h->P.veh;
  K.N = h->P.N;
  K.max_vel_ref_diff = h->P.max_vel_ref_diff;
  std::memcpy(K.ekf.Q, h->ekf_cfg.Q, sizeof(K.ekf.Q));
  std::memcpy(K.ekf.x_min, h->ekf_cfg.x_min, sizeof(K.ekf.x_min));
  std::memcpy(K.ekf.x_max, h->ekf_cfg.x_max, sizeof(K.ekf.x_max));
  // the two spans by lmpc_ekf_update_batch's expression, from the clock two such calls would have kept
  K.dt_vel = (double)(io->t_vel_ns - h->ekf_ns) * 1e-9;
  K.dt_pose = (double)(io->t_pose_ns - io->t_vel_ns) * 1e-9;
  HIP_TRY(h, lmpc_estimated_launch(h->stream, K, h->ekf, *track, spline->view, *io));
  h->ekf_ns = io->t_pose_ns;
  return LMPC_OK;
}

}  // extern "C"

// ---- batched vanilla controller, one per car (csrc/lmpc_vanilla.h, csrc/lmpc_vanilla_kernel.hip) ----
namespace {
// what every call but create and destroy checks first: a store, and the store's batch
int vanilla_check(lmpc_handle* h, int32_t batch, const char* who) {
  if (!h->vanilla.batch) return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": no controller (lmpc_vanilla_create)");
  if (batch != h->vanilla.batch)
    return fail(h, LMPC_ERR_ARGUMENT, std::string(who) + ": batch " + std::to_string(batch) + ", the store holds " + std::to_string(h->vanilla.batch));
  return LMPC_OK;
}
}  // namespace

extern "C" {

int lmpc_vanilla_destroy(lmpc_handle* h) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!h->vanilla.batch) return LMPC_OK;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  h->vanilla_pid.release();
  h->vanilla = lmpc_vanilla_store{};
  return LMPC_OK;
}

int lmpc_vanilla_create(lmpc_handle* h, int32_t batch, const lmpc_vanilla_config* cfg) {
  if (!h) return LMPC_ERR_ARGUMENT;
  if (!cfg) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_vanilla_create: null config");
  if (batch < 1 || batch > (1 << 24)) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_vanilla_create: batch outside 1 .. 2^24");
  if (!(cfg->dt > 0.0) || !std::isfinite(cfg->dt)) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_vanilla_create: dt must be positive and finite");
  if (!(cfg->min_lookahead_distance > 0.0) || !(cfg->min_lookahead_distance <= cfg->max_lookahead_distance))
    return fail(h, LMPC_ERR_ARGUMENT, "lmpc_vanilla_create: needs 0 < min_lookahead_distance <= max_lookahead_distance");
  if (!(cfg->min_i <= cfg->max_i)) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_vanilla_create: min_i > max_i");
  if (!(cfg->min_cmd <= cfg->max_cmd)) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_vanilla_create: min_cmd > max_cmd");
  const int rc0 = lmpc_vanilla_destroy(h);
  if (rc0 != LMPC_OK) return rc0;
  HIP_TRY(h, hipSetDevice(h->device));
  dev_buf<double> pid;  // a local owner: a refused allocation leaves the handle without a controller
  HIP_TRY_AS(h, "lmpc_vanilla_create", pid.alloc((size_t)3 * (size_t)batch));
  HIP_TRY_AS(h, "lmpc_vanilla_create", hipMemsetAsync(pid.get(), 0, (size_t)3 * (size_t)batch * sizeof(double), h->stream));
  HIP_TRY_AS(h, "lmpc_vanilla_create", hipStreamSynchronize(h->stream));
  h->vanilla_pid = std::move(pid);
  h->vanilla.batch = batch;
  h->vanilla.cfg = *cfg;
  h->vanilla.pid = h->vanilla_pid.get();
  return LMPC_OK;
}

int lmpc_vanilla_reset(lmpc_handle* h, int32_t batch, const double* integral) {
  if (!h) return LMPC_ERR_ARGUMENT;
  const int rc = vanilla_check(h, batch, "lmpc_vanilla_reset");
  if (rc != LMPC_OK) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t row = (size_t)batch * sizeof(double);
  HIP_TRY(h, hipMemsetAsync(h->vanilla.pid, 0, 3 * row, h->stream));
  if (integral) HIP_TRY(h, hipMemcpyAsync(h->vanilla.pid, integral, row, hipMemcpyDeviceToDevice, h->stream));
  return LMPC_OK;
}

int lmpc_vanilla_get(lmpc_handle* h, int32_t batch, double* integral, double* error, double* last_error) {
  if (!h) return LMPC_ERR_ARGUMENT;
  const int rc = vanilla_check(h, batch, "lmpc_vanilla_get");
  if (rc != LMPC_OK) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t row = (size_t)batch * sizeof(double);
  double* const dst[3] = {integral, error, last_error};
  for (int k = 0; k < 3; ++k)
    if (dst[k]) HIP_TRY(h, hipMemcpyAsync(dst[k], h->vanilla.pid + (size_t)k * batch, row, hipMemcpyDeviceToDevice, h->stream));
  return LMPC_OK;
}

int lmpc_vanilla_solve_batch(lmpc_handle* h, int32_t batch, const lmpc_spline_track* track, const double* x_ic, const double* vel_ref,
                             double speed_scale, double* u_out, double* u_model, int32_t* flags) {
  if (!h) return LMPC_ERR_ARGUMENT;
  int rc = vanilla_check(h, batch, "lmpc_vanilla_solve_batch");
  if (rc != LMPC_OK) return rc;
  rc = spline_track_check(h, track, "lmpc_vanilla_solve_batch");
  if (rc != LMPC_OK) return rc;
  if (!x_ic || !u_out) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_vanilla_solve_batch: null pointer");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, lmpc_vanilla_launch_solve(h->stream, h->vanilla, h->P.veh, track->view, batch, x_ic, vel_ref, speed_scale, u_out, u_model, flags));
  return LMPC_OK;
}

int lmpc_vanilla_rollout_batch(lmpc_handle* h, int32_t batch, const lmpc_spline_track* track, const lmpc_track* table, double* x, int32_t periods,
                               double dt_sim, int32_t n_sub, double speed_scale, double* X_log, double* U_log, double* k_log, double* distance,
                               double* worst_excess, int32_t* flags) {
  if (!h) return LMPC_ERR_ARGUMENT;
  int rc = vanilla_check(h, batch, "lmpc_vanilla_rollout_batch");
  if (rc != LMPC_OK) return rc;
  rc = spline_track_check(h, track, "lmpc_vanilla_rollout_batch");
  if (rc != LMPC_OK) return rc;
  if (!track_ok(table)) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_vanilla_rollout_batch: null or empty track table");
  if (!x) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_vanilla_rollout_batch: null pointer");
  if (periods < 1 || n_sub < 1) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_vanilla_rollout_batch: periods and n_sub must be at least 1");
  if (!(dt_sim > 0.0) || !std::isfinite(dt_sim)) return fail(h, LMPC_ERR_ARGUMENT, "lmpc_vanilla_rollout_batch: dt_sim must be positive and finite");
  HIP_TRY(h, hipSetDevice(h->device));
  const lmpc_vanilla_rollout_io io{x, X_log, U_log, k_log, distance, worst_excess, flags};
  HIP_TRY(h, lmpc_vanilla_launch_rollout(h->stream, h->vanilla, h->P.veh, track->view, *table, batch, periods, dt_sim, n_sub, speed_scale, io));
  return LMPC_OK;
}

// the rollout of a fleet: a plant per car, the fleet recorder in the period loop (include/lmpc_hip_vanilla_fleet.h)
int lmpc_vanilla_rollout_fleet_batch(lmpc_handle* h, int32_t batch, const lmpc_spline_track* track, const lmpc_track* table,
                                     const lmpc_vanilla_fleet_rollout* io) {
  if (!h) return LMPC_ERR_ARGUMENT;
  const std::string who = "lmpc_vanilla_rollout_fleet_batch";
  int rc = vanilla_check(h, batch, who.c_str());
  if (rc != LMPC_OK) return rc;
  rc = spline_track_check(h, track, who.c_str());
  if (rc != LMPC_OK) return rc;
  if (!track_ok(table)) return fail(h, LMPC_ERR_ARGUMENT, who + ": null or empty track table");
  if (!io || !io->x) return fail(h, LMPC_ERR_ARGUMENT, who + ": io or io->x is NULL");
  if (io->periods < 1 || io->n_sub < 1) return fail(h, LMPC_ERR_ARGUMENT, who + ": periods and n_sub must be at least 1");
  if (!(io->dt_sim > 0.0) || !std::isfinite(io->dt_sim)) return fail(h, LMPC_ERR_ARGUMENT, who + ": dt_sim must be positive and finite");
  if (io->plant != LMPC_VANILLA_PLANT_HANDLE && io->plant != LMPC_VANILLA_PLANT_CARS && io->plant != LMPC_VANILLA_PLANT_DTRACK)
    return fail(h, LMPC_ERR_ARGUMENT, who + ": plant is none of LMPC_VANILLA_PLANT_HANDLE, _CARS, _DTRACK");
  if (io->record != LMPC_VANILLA_RECORD_NONE && io->record != LMPC_VANILLA_RECORD_APPLIED && io->record != LMPC_VANILLA_RECORD_ARRIVED)
    return fail(h, LMPC_ERR_ARGUMENT, who + ": record is none of LMPC_VANILLA_RECORD_NONE, _APPLIED, _ARRIVED");
  if (io->period0 < 0) return fail(h, LMPC_ERR_ARGUMENT, who + ": period0 is negative");
  lmpc_vanilla_fleet_io fx{nullptr, io->u_prev, io->record == LMPC_VANILLA_RECORD_ARRIVED, (long long)io->period0, io->dt};
  if (io->plant == LMPC_VANILLA_PLANT_CARS) {
    if (!h->cars_B) return fail(h, LMPC_ERR_ARGUMENT, who + ": no car table (lmpc_cars_set_vehicles)");
    if (h->cars_B != batch)
      return fail(h, LMPC_ERR_ARGUMENT, who + ": batch " + std::to_string(batch) + " is not the car table's " + std::to_string(h->cars_B));
    fx.table = h->cars_tab.get();
  } else if (io->plant == LMPC_VANILLA_PLANT_DTRACK) {
    if (!h->dtrack_B) return fail(h, LMPC_ERR_ARGUMENT, who + ": no double-track table (lmpc_dtrack_set_vehicles)");
    if (h->dtrack_B != batch)
      return fail(h, LMPC_ERR_ARGUMENT, who + ": batch " + std::to_string(batch) + " is not the double-track table's " + std::to_string(h->dtrack_B));
    fx.table = h->dtrack_tab.get();
  }
  const bool record = io->record != LMPC_VANILLA_RECORD_NONE;
  if (record) {
    rc = fleet_check(h, batch, who.c_str());
    if (rc != LMPC_OK) return rc;
    if (!(io->dt > 0.0) || !std::isfinite(io->dt)) return fail(h, LMPC_ERR_ARGUMENT, who + ": dt must be positive and finite when recording");
    if (fx.arrived && !io->u_prev) return fail(h, LMPC_ERR_ARGUMENT, who + ": LMPC_VANILLA_RECORD_ARRIVED needs u_prev");
  }
  HIP_TRY(h, hipSetDevice(h->device));
  if (record) h->fleet_L = table->L;  // what the query unrolls the laps by, as lmpc_fleet_ss_record_batch notes it
  const lmpc_vanilla_rollout_io rio{io->x, io->X_log, io->U_log, io->k_log, io->distance, io->worst_excess, io->flags};
  HIP_TRY(h, lmpc_vanilla_launch_fleet(h->stream, h->vanilla, h->P.veh, track->view, *table, batch, io->periods, io->dt_sim, io->n_sub,
                                       io->speed_scale, rio, io->plant, record, fx, h->fleet));
  return LMPC_OK;
}

}  // extern "C"
