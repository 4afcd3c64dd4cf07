// lmpc_wave.hip.h -- the single-wavefront primitives every phase of the solve is written in.
// Holds: the phase clocks of the profiling build (Prof, PT_*), wavefront fences, values moved to scalar registers (uni, uni_ptr),
// lane / group / row broadcasts, DPP reductions, pair_exchange and wave_sum_split, frcp / frsqrt / rfma, and the scheduling pins
// (ISSUE_ORDER, AFTER_VALUE, FRESH_LANE, CHAIN_PRIO_*: the last two expect the caller's Lds handle to be called `L`).
// Needs: the HIP runtime header and <utility> only.  Included by lmpc_solve_kernel.hip (all three translation units).
#ifndef LMPC_WAVE_HIP_H_
#define LMPC_WAVE_HIP_H_

// Optional per-phase cycle accounting (make prof -> -DLMPC_PHASE_TIMING): one s_memtime read per
// phase boundary, per-wave totals written over kkt_out as [16][B] doubles, four words of bookkeeping behind them and buckets 16 .. 19
// behind those (the caller allocates 24 rows).  Buckets 13 .. 15, 18 and 19 of a KS = 0 kernel are the active-set polish's own clocks
// (factorisation, backward sweeps, forward sweeps, row work with the save-area traffic, calls), which the callee hands back in its
// result and which are ALSO inside the caller's bucket 7; 16 and 17 are the start point's factorisation and rollout.
#ifdef LMPC_PHASE_TIMING
struct Prof {
  long long acc[20];
  long long t, w0;
};
#define PT_DECL Prof pf; { for (int k = 0; k < 20; ++k) pf.acc[k] = 0; pf.t = __builtin_readcyclecounter(); pf.w0 = wall_clock64(); }
#define PT_MARK(k) { const long long pt_n = __builtin_readcyclecounter(); pf.acc[k] += pt_n - pf.t; pf.t = pt_n; }
#else
struct Prof {};
#define PT_DECL Prof pf;
#define PT_MARK(k)
#endif

// The workgroup is a single wavefront and the LDS executes one wave's DS instructions in issue order, so cross-lane
// exchange through LDS needs no s_barrier and no wait for the write to retire: only the compiler must not move memory
// operations across the exchange point.  __builtin_amdgcn_wave_barrier alone does not say that -- it is declared as not
// touching memory, so around a store that only SOME lanes execute (`if (lane < 6) T[..] = ..`) the IR-level passes may
// still schedule the other lanes' later loads of those cells, on the not-taken path, ahead of the taken path's stores:
// the readers then see the previous content (seen once on the terminal block of the learning problem: results changed
// from process to process).  Release / acquire fences at WAVEFRONT scope around the barrier pin the order; at that scope
// they emit no cache action and no wait.
__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ void wave_sync() { wave_fence(); }

// A value that is the same in every lane, moved to scalar registers (v_readfirstlane): the solver's
// wave-wide scalars (mu, step lengths, sigma, ...) then cost no vector registers while they are carried
// across the Riccati sweeps, and feed the VALU as scalar operands.
__device__ __forceinline__ double uni(double x) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
}
__device__ __forceinline__ float uni(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }

// Lane k's value of a wave-distributed number as a wave-uniform scalar (v_readlane_b32; the result lives in SGPRs
// and feeds the FMAs as a scalar operand).
__device__ __forceinline__ double lane_bcast(double v, int k) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), k);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float lane_bcast(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }

// ds_swizzle bit mode: source lane = (lane & 0x18) | K, i.e. lane K of each group of 8 (PATTERN = 0x18 | K << 5)
template <int PATTERN>
__device__ __forceinline__ double group_bcast(double v) {
  return __hiloint2double(__builtin_amdgcn_ds_swizzle(__double2hiint(v), PATTERN), __builtin_amdgcn_ds_swizzle(__double2loint(v), PATTERN));
}
template <int PATTERN>
__device__ __forceinline__ float group_bcast(float v) { return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), PATTERN)); }

// Wave reductions on the VALU (DPP), not through the LDS crossbar (ds_bpermute): the LDS pipeline is this kernel's
// tightest resource and a 6-step bpermute chain costs ~460 cycles of latency against ~130 here.  Four row_ror steps
// leave every lane of a 16-lane row with the row's total, row_bcast15 / row_bcast31 fold the rows into lane 63.
//
// The moves carry NO "old" operand (__builtin_amdgcn_mov_dpp, not update_dpp with an identity): a lane the DPP does not write
// then holds an unspecified value, and the compiler no longer materialises an identity (two v_mov_b32 and usually an s_nop for
// the DPP read hazard) in front of every step of every reduced value.  That is sound only where every lane that is READ
// afterwards is WRITTEN at every step.  The lane argument for wave_reduce_n, whose only read is lane 63:
//   steps 1 - 4, row_ror 8 / 4 / 2 / 1, row mask 0xf: every lane has a source in its own row and every row is enabled;
//   step 5, row_bcast15, row mask 0xa: writes rows 1 and 3 (lanes 16 .. 31 from lane 15, lanes 48 .. 63 from lane 47);
//           lane 63 is in row 3; its source, lane 47, is read as steps 1 - 4 left it (a DPP reads the value before its own step);
//   step 6, row_bcast31, row mask 0xc: writes rows 2 and 3 from lane 31; lane 63 is in row 3; lane 31 is in row 1, written by
//           steps 1 - 5.
// Lanes of rows 0 and 2 combine an unspecified value in step 5 (rows 0 and 1 in step 6) and nobody reads them afterwards: a
// new reader of any lane but 63 has to bring the identity back.  pair_exchange below runs full masks on controls that give
// every lane a source, so every lane is written.
//
// The association order the steps produce is a contract (tests/cpp/test_wave_reduce.hip restates it on the host and compares
// bits).  With x[r][j] lane j of row r, t = f(v, moved) at every step, and row_ror:n giving lane j the value of lane
// (j - n) mod 16 of its row:
//   a[j] = f(x[j], x[j - 8]);  b[j] = f(a[j], a[j - 4]);  c[j] = f(b[j], b[j - 2]);  R_r = f(c[15], c[14])    (indices mod 16)
//   result = f(f(R_3, R_2), f(R_1, R_0))
// f's first argument is always the lane's own value, the second the moved one (fmax / fmin of a NaN and a number is the number).
//
// KEEP_ID = true is the form with the identity as "old" (unwritten lanes keep it): the same bits in lane 63 and in every
// exchanged lane, for the instantiations whose register allocation the shorter form makes worse (lmpc_reduce_identity,
// lmpc_solve_layout.hip.h).
template <int CTRL, int ROW_MASK, bool KEEP_ID = false>
__device__ __forceinline__ double dpp_move(double x, double identity) {
  if constexpr (KEEP_ID) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(identity), __double2loint(x), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(identity), __double2hiint(x), CTRL, ROW_MASK, 0xf, false);
    return __hiloint2double(hi, lo);
  } else {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(x), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(x), CTRL, ROW_MASK, 0xf, false);
    return __hiloint2double(hi, lo);
  }
}
template <int CTRL, int ROW_MASK, bool KEEP_ID = false>
__device__ __forceinline__ float dpp_move(float x, float identity) {
  if constexpr (KEEP_ID) return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(identity), __float_as_int(x), CTRL, ROW_MASK, 0xf, false));
  else return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), CTRL, ROW_MASK, 0xf, false));
}
#define DPP_ROW_ROR(n) (0x120 + (n))
#define DPP_ROW_BCAST15 0x142
#define DPP_ROW_BCAST31 0x143
struct op_sum {
  template <typename real> static __device__ __forceinline__ real id() { return real(0); }
  template <typename real> static __device__ __forceinline__ real f(real a, real b) { return a + b; }
};
struct op_max {
  template <typename real> static __device__ __forceinline__ real id() { return -real(INFINITY); }
  template <typename real> static __device__ __forceinline__ real f(real a, real b) { return fmax(a, b); }
};
struct op_min {
  template <typename real> static __device__ __forceinline__ real id() { return real(INFINITY); }
  template <typename real> static __device__ __forceinline__ real f(real a, real b) { return fmin(a, b); }
};
// NV independent reductions in lock-step (their steps interleave); results as wave-uniform scalars
template <class OP, int NV, bool KEEP_ID = false, typename real>
__device__ __forceinline__ void wave_reduce_n(real (&v)[NV]) {
  const real id = OP::template id<real>();
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = OP::f(v[k], dpp_move<DPP_ROW_ROR(8), 0xf, KEEP_ID>(v[k], id));
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = OP::f(v[k], dpp_move<DPP_ROW_ROR(4), 0xf, KEEP_ID>(v[k], id));
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = OP::f(v[k], dpp_move<DPP_ROW_ROR(2), 0xf, KEEP_ID>(v[k], id));
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = OP::f(v[k], dpp_move<DPP_ROW_ROR(1), 0xf, KEEP_ID>(v[k], id));
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = OP::f(v[k], dpp_move<DPP_ROW_BCAST15, 0xa, KEEP_ID>(v[k], id));
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = OP::f(v[k], dpp_move<DPP_ROW_BCAST31, 0xc, KEEP_ID>(v[k], id));
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = lane_bcast(v[k], 63);
}
#undef DPP_ROW_ROR
#undef DPP_ROW_BCAST15
#undef DPP_ROW_BCAST31
template <bool KEEP_ID = false, typename real>
__device__ __forceinline__ real wave_sum(real x) {
  real v[1] = {x};
  wave_reduce_n<op_sum, 1, KEEP_ID>(v);
  return v[0];
}
template <bool KEEP_ID = false, typename real>
__device__ __forceinline__ real wave_max(real x) {
  real v[1] = {x};
  wave_reduce_n<op_max, 1, KEEP_ID>(v);
  return v[0];
}
template <bool KEEP_ID = false, typename real>
__device__ __forceinline__ real wave_min(real x) {
  real v[1] = {x};
  wave_reduce_n<op_min, 1, KEEP_ID>(v);
  return v[0];
}
template <int NV, bool KEEP_ID = false, typename real>
__device__ __forceinline__ void wave_sum_n(real (&v)[NV]) {
  wave_reduce_n<op_sum, NV, KEEP_ID>(v);
}

// Exchange with the partner lane that differs in bit BIT of the lane number (and, for bits 2 and 3, in the bits below:
// the row mirrors are the involutions DPP offers there) -- every pairing used by wave_sum_split below.
template <int BIT, bool KEEP_ID = false>
__device__ __forceinline__ double pair_exchange(double x) {
  if constexpr (BIT == 5) return __shfl_xor(x, 32, 64);
  if constexpr (BIT == 4)  // ds_swizzle, bit mode: and 0x1f, or 0, xor 0x10
    return __hiloint2double(__builtin_amdgcn_ds_swizzle(__double2hiint(x), 0x401F), __builtin_amdgcn_ds_swizzle(__double2loint(x), 0x401F));
  if constexpr (BIT == 3) return dpp_move<0x140, 0xf, KEEP_ID>(x, 0.0);  // row_mirror
  if constexpr (BIT == 2) return dpp_move<0x141, 0xf, KEEP_ID>(x, 0.0);  // row_half_mirror
  if constexpr (BIT == 1) return dpp_move<0x4E, 0xf, KEEP_ID>(x, 0.0);   // quad_perm [2,3,0,1]
  return dpp_move<0xB1, 0xf, KEEP_ID>(x, 0.0);                            // quad_perm [1,0,3,2]
}
template <int BIT, bool KEEP_ID = false>
__device__ __forceinline__ float pair_exchange(float x) { return (float)pair_exchange<BIT, KEEP_ID>((double)x); }

// Many sums at once, for NV up to 32 (the safe-set block reduces 35 per iteration): instead of NV full reductions, each
// step pairs the lanes across one bit of the lane number and SPLITS the values between the partners -- the lane with
// the bit clear keeps the lower half (adding its partner's contributions), the other the upper half -- so the work
// halves with every step: P/2 + P/4 + ... exchanges for P values instead of 6 P.  After log2 P steps lane l holds the
// partial total of value l >> (6 - log2 P) over its group; plain pairwise sums over the remaining bits finish it.
template <int NV, bool KEEP_ID = false, typename real>
__device__ __forceinline__ void wave_sum_split(real (&v)[NV], int lane) {
  constexpr int P = NV <= 2 ? 2 : NV <= 4 ? 4 : NV <= 8 ? 8 : NV <= 16 ? 16 : 32;
  constexpr int LOGP = P == 2 ? 1 : P == 4 ? 2 : P == 8 ? 3 : P == 16 ? 4 : 5;
  static_assert(NV <= 32, "wave_sum_split handles up to 32 values");
  real a[P];
#pragma unroll
  for (int k = 0; k < P; ++k) a[k] = k < NV ? v[k] : real(0);
  auto split = [&](auto bit_c, auto half_c) {
    constexpr int BIT = decltype(bit_c)::value, H = decltype(half_c)::value;
    const bool up = (lane >> BIT) & 1;
#pragma unroll
    for (int k = 0; k < H; ++k) {
      const real keep = up ? a[k + H] : a[k];
      const real send = up ? a[k] : a[k + H];
      a[k] = keep + pair_exchange<BIT, KEEP_ID>(send);
    }
  };
  auto fold = [&](auto bit_c) {
    constexpr int BIT = decltype(bit_c)::value;
    a[0] = a[0] + pair_exchange<BIT, KEEP_ID>(a[0]);
  };
  using std::integral_constant;
  // bits 5, 4, 3, 2, 1 carry the splits while more than one value is left; the rest are plain sums
  if constexpr (LOGP >= 1) split(integral_constant<int, 5>{}, integral_constant<int, P / 2>{}); else fold(integral_constant<int, 5>{});
  if constexpr (LOGP >= 2) split(integral_constant<int, 4>{}, integral_constant<int, P / 4>{}); else fold(integral_constant<int, 4>{});
  if constexpr (LOGP >= 3) split(integral_constant<int, 3>{}, integral_constant<int, (P / 8 > 0 ? P / 8 : 1)>{}); else fold(integral_constant<int, 3>{});
  if constexpr (LOGP >= 4) split(integral_constant<int, 2>{}, integral_constant<int, (P / 16 > 0 ? P / 16 : 1)>{}); else fold(integral_constant<int, 2>{});
  if constexpr (LOGP >= 5) split(integral_constant<int, 1>{}, integral_constant<int, 1>{}); else fold(integral_constant<int, 1>{});
  fold(integral_constant<int, 0>{});
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = lane_bcast(a[0], k << (6 - LOGP));
}

// 1/x: hardware v_rcp seed + one Newton step (full accuracy for normal x); replaces the ~12-instruction IEEE
// division sequence in the per-row arithmetic.
__device__ __forceinline__ double frcp(double x) {
  double r = __builtin_amdgcn_rcp(x);
  return __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
}
__device__ __forceinline__ float frcp(float x) {
  float r = __builtin_amdgcn_rcpf(x);
  return __builtin_fmaf(__builtin_fmaf(-x, r, 1.0f), r, r);
}

// 1/sqrt(x): hardware v_rsq seed + Newton steps y <- y + y (1 - x y^2)/2 (two in double: the seed carries ~26 bits);
// the IEEE sqrt + division pair it replaces is ~70 dependent instructions, ten times per terminal factorisation.
__device__ __forceinline__ double frsqrt(double x) {
  double y = __builtin_amdgcn_rsq(x);
  y = __builtin_fma(0.5 * y, __builtin_fma(-x * y, y, 1.0), y);
  return __builtin_fma(0.5 * y, __builtin_fma(-x * y, y, 1.0), y);
}
__device__ __forceinline__ float frsqrt(float x) {
  const float y = __builtin_amdgcn_rsqf(x);
  return __builtin_fmaf(0.5f * y, __builtin_fmaf(-x * y, y, 1.0f), y);
}

__device__ __forceinline__ double rfma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float rfma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// Pin the issue order of LDS traffic: one wave's DS instructions return in issue order, so the read a
// serial chain waits for must be queued ahead of the operand prefetch of the following stage.
#define ISSUE_ORDER() __builtin_amdgcn_sched_barrier(0)
// The serial stage chains (factorisation, sweeps) at a higher issue priority than the row phases of the wave they share a SIMD
// with (s_setprio): the chain's next instruction is the one a solve waits for, the row phases are throughput work that fills in.
// Two-waves-per-SIMD kernels only (alone on its SIMD a wave has nobody to yield to: +0.5 %): headline kernel -1.5 %, pipelined
// +1.4 %, one batch at a time -1.9 %, the mixed learning kernel -1.1 %; same bits (profiles/r04_row_phases.md).
#define LMPC_CHAIN_PRIO 3
// (the learning problem's terminal elimination is another serial chain; raising its priority the same way was measured in round 4 and
//  bought nothing: profiles/r04_row_phases.md)
#define CHAIN_PRIO_ENTER() do { if (LMPC_CHAIN_PRIO && L.chain_prio) __builtin_amdgcn_s_setprio(LMPC_CHAIN_PRIO); } while (0)
#define CHAIN_PRIO_LEAVE() do { if (LMPC_CHAIN_PRIO && L.chain_prio) __builtin_amdgcn_s_setprio(0); } while (0)
// ... and the other way round: value x is complete before any later memory operation is issued (an
// empty asm that consumes x and clobbers memory), used to keep a prefetch behind the last use of the
// registers it overwrites.
#define AFTER_VALUE(x) asm volatile("" : "+v"(x) : : "memory")
// The lane number as a value the optimiser cannot see through: everything a sweep derives from it (row / column indices,
// LDS addresses, 0/1 multipliers, predicates) is then computed where the sweep starts -- a dozen VALU instructions -- instead
// of once at the top of the kernel and kept alive over the whole iteration, which at the register limit means spilled and
// reloaded from scratch (or from VGPR lanes, for the predicates) inside the sweep's preamble, one wait per reload.  Measured per
// instantiation in round 4 -- what it does to the register allocation of a 3000-line kernel is not monotone -- and it paid in
// every one (profiles/r04_polish_forms.md; round 4 also bisected a miscompute with a per-sweep mask, profiles/r04_d70_bisect.md).
#define FRESH_LANE(l) asm volatile("" : "+v"(l))

// Lane K of every 16-lane row to the whole row (DPP row_newbcast, gfx90a+; v_mov_b64_dpp for doubles): a register-to-
// register broadcast.  bound_ctrl:1 with full row / bank masks tells the compiler that the tied "old" operand is never
// read, so it is not materialised (with bound_ctrl:0 every broadcast costs a v_mov of a constant first -- a fifth of the
// sweeps' VALU instructions).  (An inline-asm form of the same instructions measured the same speed and was NOT safe: in
// the most register-starved instantiation, KQ = 14 with KS = 3, it gave wrong and run-to-run different results that wider
// wait states did not cure, while this builtin form is bitwise reproducible there -- the compiler has to see DPP.)
template <int K>
__device__ __forceinline__ double row_bcast(double v) { return __builtin_amdgcn_update_dpp(0.0, v, 0x150 + K, 0xf, 0xf, true); }
template <int K>
__device__ __forceinline__ float row_bcast(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x150 + K, 0xf, 0xf, true));
}
template <typename real>
__device__ __forceinline__ void row_bcast6(real v, real (&o)[6]) {
  o[0] = row_bcast<0>(v); o[1] = row_bcast<1>(v); o[2] = row_bcast<2>(v);
  o[3] = row_bcast<3>(v); o[4] = row_bcast<4>(v); o[5] = row_bcast<5>(v);
}
template <typename real>
__device__ __forceinline__ void row_bcast8(real v, real (&o)[8]) {
  o[0] = row_bcast<0>(v); o[1] = row_bcast<1>(v); o[2] = row_bcast<2>(v); o[3] = row_bcast<3>(v);
  o[4] = row_bcast<4>(v); o[5] = row_bcast<5>(v); o[6] = row_bcast<6>(v); o[7] = row_bcast<7>(v);
}
template <typename real>
__device__ __forceinline__ void row_bcast67(real v, real& a, real& b) {  // lanes 6 and 7
  a = row_bcast<6>(v);
  b = row_bcast<7>(v);
}

// LDS byte addresses for the stage chains that walk them (the CHAIN_PINNED form, lmpc_solve_layout.hip.h): the address of a cell of the workgroup's
// block as a 32-bit number, a typed LDS pointer back from it (its constant indices become the DS instructions' immediate offsets), and
// the pin that keeps an address a register of its own from stage to stage -- left to itself the optimiser rewrites the walk as
// base + index * stride and forms every address again at its use.
#define LMPC_LDS __attribute__((address_space(3)))
template <typename T>
__device__ __forceinline__ unsigned lds_addr(const T* p) { return (unsigned)(unsigned long long)(LMPC_LDS const T*)p; }
template <typename T>
__device__ __forceinline__ LMPC_LDS T* lds_at(unsigned a) { return (LMPC_LDS T*)(unsigned long long)a; }
#define CHAIN_ADDR_PIN(a) asm volatile("" : "+v"(a))
// ... and, for the addresses of 16-byte rows, what the pin hides: that they are 16-byte aligned (ds_read_b128, not two ds_read_b64)
#define CHAIN_ADDR_PIN16(a) do { CHAIN_ADDR_PIN(a); __builtin_assume(((a) & 15u) == 0u); } while (0)

__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
template <typename T>
__device__ __forceinline__ T* uni_ptr(T* p) {
  const unsigned long long v = reinterpret_cast<unsigned long long>(p);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return reinterpret_cast<T*>(((unsigned long long)hi << 32) | lo);
}

#endif
