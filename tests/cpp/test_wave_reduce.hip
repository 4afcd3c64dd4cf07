// The wave reductions of csrc/lmpc_wave.hip.h on one 64-lane wave against a host re-statement of their butterflies, bit for bit:
// wave_sum, wave_max, wave_min, wave_sum_n<2>, wave_sum_n<3>, wave_sum_split<7> and <32>, in double and in float.
// The association order is the header's contract (its comment above dpp_move); the host side below follows it lane by lane, keeps
// track of which lanes a step writes, and refuses a result that was formed from a lane no step wrote -- the lane argument that lets
// the moves run without an identity.  The sum inputs are chosen (and checked here, on the host) so that other association orders
// give other bits.  Every f is commutative, so a row's total does not depend on the direction of row_ror; the emulation rotates
// the way the ISA manual states it (lane j reads lane j - n of its row).
// usage: test_wave_reduce      prints one line per check and PASS
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "lmpc_wave.hip.h"

namespace {

constexpr int SUM_SETS = 32, MAX_SETS = 4;
constexpr int N_OUT = SUM_SETS + 2 * MAX_SETS + 2 + 3 + 7 + 32;

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

// in: [SUM_SETS + MAX_SETS][64], out: [N_OUT]
template <typename real>
__global__ void __launch_bounds__(64) reduce_kernel(const real* __restrict__ in, real* __restrict__ out) {
  const int lane = threadIdx.x;
  real x[SUM_SETS], m[MAX_SETS];
#pragma unroll
  for (int s = 0; s < SUM_SETS; ++s) x[s] = in[s * 64 + lane];
#pragma unroll
  for (int s = 0; s < MAX_SETS; ++s) m[s] = in[(SUM_SETS + s) * 64 + lane];
  real r[N_OUT];
  int o = 0;
#pragma unroll
  for (int s = 0; s < SUM_SETS; ++s) r[o++] = wave_sum(x[s]);
#pragma unroll
  for (int s = 0; s < MAX_SETS; ++s) r[o++] = wave_max(m[s]);
#pragma unroll
  for (int s = 0; s < MAX_SETS; ++s) r[o++] = wave_min(m[s]);
  real v2[2] = {x[0], x[1]};
  wave_sum_n<2>(v2);
  r[o++] = v2[0]; r[o++] = v2[1];
  real v3[3] = {x[2], x[3], x[4]};
  wave_sum_n<3>(v3);
  r[o++] = v3[0]; r[o++] = v3[1]; r[o++] = v3[2];
  real v7[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) v7[k] = x[k];
  wave_sum_split<7>(v7, lane);
#pragma unroll
  for (int k = 0; k < 7; ++k) r[o++] = v7[k];
  real v32[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) v32[k] = x[k];
  wave_sum_split<32>(v32, lane);
#pragma unroll
  for (int k = 0; k < 32; ++k) r[o++] = v32[k];
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N_OUT; ++k) out[k] = r[k];
  }
}

// ---- the host re-statement ----
enum Op { SUM, MAX, MIN };
// v_max / v_min as the hardware orders them: a NaN loses to a number, -0 is below +0
template <typename real>
real host_f(Op op, real a, real b) {
  if (op == SUM) return a + b;
  if (std::isnan(a)) return b;
  if (std::isnan(b)) return a;
  if (a == b) return (op == MAX) == std::signbit(a) ? b : a;   // equal numbers or zeros of either sign: max takes the one without the sign bit
  return op == MAX ? (a > b ? a : b) : (a < b ? a : b);
}

// wave_reduce_n, one value: six steps over 64 lanes; `good` follows which lanes hold a value every step so far has defined
template <typename real>
bool host_reduce(Op op, const real* x, real* result, real* rows = nullptr) {
  real v[64];
  bool good[64];
  for (int l = 0; l < 64; ++l) { v[l] = x[l]; good[l] = true; }
  auto step = [&](auto src_of, int row_mask) {
    real nv[64];
    bool ng[64];
    for (int l = 0; l < 64; ++l) {
      const int src = src_of(l);
      const bool written = ((row_mask >> (l >> 4)) & 1) && src >= 0;
      nv[l] = written ? host_f(op, v[l], v[src]) : v[l];
      ng[l] = written && good[l] && good[src];
    }
    std::memcpy(v, nv, sizeof v);
    std::memcpy(good, ng, sizeof good);
  };
  for (int n : {8, 4, 2, 1}) step([n](int l) { return (l & 48) | ((l - n) & 15); }, 0xf);   // row_ror:n
  for (int r = 0; rows && r < 4; ++r) rows[r] = v[16 * r + 15];
  step([](int l) { return (l >> 4) ? (l & 48) - 1 : -1; }, 0xa);                            // row_bcast15: lane 15 of the row below
  step([](int l) { return (l >> 5) ? 31 : -1; }, 0xc);                                      // row_bcast31
  *result = v[63];
  return good[63];
}

int partner(int l, int bit) {
  switch (bit) {
    case 5: return l ^ 32;
    case 4: return l ^ 16;
    case 3: return (l & 48) | (15 - (l & 15));   // row_mirror
    case 2: return (l & 56) | (7 - (l & 7));     // row_half_mirror
    case 1: return l ^ 2;
    default: return l ^ 1;
  }
}

// wave_sum_split<NV>: splits over bits 5, 4, .. while more than one value is left, then plain pairwise sums
template <typename real>
void host_split(int NV, const real* const* x, real* result) {
  const int P = NV <= 2 ? 2 : NV <= 4 ? 4 : NV <= 8 ? 8 : NV <= 16 ? 16 : 32;
  int LOGP = 0;
  while ((1 << LOGP) < P) ++LOGP;
  std::vector<real> a(64 * 32, real(0));
  for (int l = 0; l < 64; ++l)
    for (int k = 0; k < NV; ++k) a[l * 32 + k] = x[k][l];
  int H = P / 2;
  for (int step = 0, bit = 5; bit >= 0; ++step, --bit) {
    std::vector<real> n(a);
    if (step < LOGP) {
      for (int l = 0; l < 64; ++l) {
        const bool up = (l >> bit) & 1;
        const int p = partner(l, bit);
        for (int k = 0; k < H; ++k) {
          const real keep = up ? a[l * 32 + k + H] : a[l * 32 + k];
          const real got = up ? a[p * 32 + k + H] : a[p * 32 + k];   // the partner has the other `up`: it sends what this lane keeps
          n[l * 32 + k] = keep + got;
        }
      }
      H = H > 1 ? H / 2 : 1;
    } else {
      for (int l = 0; l < 64; ++l) n[l * 32] = a[l * 32] + a[partner(l, bit) * 32];
    }
    a.swap(n);
  }
  for (int k = 0; k < NV; ++k) result[k] = a[(k << (6 - LOGP)) * 32];
}

// other orders a sum could take, which the inputs must tell apart from the contract's
template <typename real>
real sum_serial(const real* x) {
  real s = x[0];
  for (int l = 1; l < 64; ++l) s += x[l];
  return s;
}
template <typename real>
real sum_xor_tree(const real* x, bool low_bits_first) {
  real v[64];
  std::memcpy(v, x, sizeof v);
  for (int s = 0; s < 6; ++s) {
    const int d = 1 << (low_bits_first ? s : 5 - s);
    real n[64];
    for (int l = 0; l < 64; ++l) n[l] = v[l] + v[l ^ d];
    std::memcpy(v, n, sizeof v);
  }
  return v[0];
}
template <typename real>
real sum_rows_serial(const real* x) {   // the contract's row totals, folded ((R0 + R1) + R2) + R3
  real R[4], t;
  host_reduce(SUM, x, &t, R);
  return ((R[0] + R[1]) + R[2]) + R[3];
}

template <typename real>
bool same_bits(real a, real b) { return std::memcmp(&a, &b, sizeof a) == 0; }

uint64_t rng_state;
uint64_t rng() {   // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
double unit() { return (double)(rng() >> 11) * (1.0 / 9007199254740992.0); }

template <typename real>
int run(const char* name) {
  rng_state = 20240607;
  const real inf = std::numeric_limits<real>::infinity(), qnan = std::numeric_limits<real>::quiet_NaN();
  std::vector<real> in((SUM_SETS + MAX_SETS) * 64);
  // sums: signed values with magnitudes spread over 1e-12 .. 1e12, a window of the spread per set so that no single term decides
  // every bit; signed zeros sprinkled in; set 30 is zeros of both signs only, set 31 carries +inf
  for (int s = 0; s < SUM_SETS; ++s)
    for (int l = 0; l < 64; ++l) {
      const double lo = -12.0 + 20.0 * (s % 6) / 5.0, e = lo + 4.0 * unit();
      double v = (rng() & 1 ? -1.0 : 1.0) * std::pow(10.0, e) * (1.0 + unit());
      if (s % 5 == 4 && l % 7 == 3) v = (l & 8) ? -0.0 : 0.0;
      if (s == 30) v = (rng() & 1) ? -0.0 : 0.0;
      if (s == 31 && l == 37) v = inf;
      in[s * 64 + l] = (real)v;
    }
  // max / min: the spread; the spread with both infinities, zeros of both signs and one quiet NaN; zeros of both signs only; the
  // spread with the NaN in lane 63 (the lane that is read) and another in lane 15
  for (int s = 0; s < MAX_SETS; ++s)
    for (int l = 0; l < 64; ++l) {
      double v = (rng() & 1 ? -1.0 : 1.0) * std::pow(10.0, -12.0 + 24.0 * unit());
      if (s == 1) { if (l == 5) v = inf; if (l == 50) v = -inf; if (l == 22) v = qnan; if (l == 9) v = 0.0; if (l == 41) v = -0.0; }
      if (s == 2) v = (rng() & 1) ? -0.0 : 0.0;
      if (s == 3 && (l == 63 || l == 15)) v = qnan;
      in[(SUM_SETS + s) * 64 + l] = (real)v;
    }

  // what the device must return
  std::vector<real> want(N_OUT);
  int o = 0, fails = 0, apart[4] = {0, 0, 0, 0};
  bool lanes_ok = true;
  for (int s = 0; s < SUM_SETS; ++s) {
    lanes_ok &= host_reduce(SUM, &in[s * 64], &want[o]);
    const real* x = &in[s * 64];
    if (s < 30) {   // the finite, non-trivial sets: on how many of them does each other order give other bits
      apart[0] += !same_bits(want[o], sum_serial(x));
      apart[1] += !same_bits(want[o], sum_xor_tree(x, true));
      apart[2] += !same_bits(want[o], sum_xor_tree(x, false));
      apart[3] += !same_bits(want[o], sum_rows_serial(x));
    }
    ++o;
  }
  for (int s = 0; s < MAX_SETS; ++s) lanes_ok &= host_reduce(MAX, &in[(SUM_SETS + s) * 64], &want[o++]);
  for (int s = 0; s < MAX_SETS; ++s) lanes_ok &= host_reduce(MIN, &in[(SUM_SETS + s) * 64], &want[o++]);
  for (int s = 0; s < 5; ++s) lanes_ok &= host_reduce(SUM, &in[s * 64], &want[o++]);   // sum_n<2> on sets 0, 1; sum_n<3> on 2, 3, 4
  const real* sets[32];
  for (int k = 0; k < 32; ++k) sets[k] = &in[k * 64];
  host_split(7, sets, &want[o]);
  o += 7;
  host_split(32, sets, &want[o]);
  o += 32;
  int split_apart = 0;   // the split's order is not the butterfly's: the same sets, other bits
  for (int k = 0; k < 30; ++k) split_apart += !same_bits(want[SUM_SETS + 2 * MAX_SETS + 5 + 7 + k], want[k]);
  std::printf("%s: host: lane 63 formed from written lanes only: %s; of 30 sum sets, other bits than the contract's order: serial %d, xor tree from bit 0 %d, "
              "xor tree from bit 5 %d, rows folded serially %d, wave_sum_split<32> %d\n", name, lanes_ok ? "yes" : "NO", apart[0], apart[1], apart[2], apart[3], split_apart);
  // (two orders often round to the same bits on one set -- the serial fold of the rows differs from the contract in two additions
  //  only; an order that differed on none of the 30 would pass for the contract's, so each has to show on five sets at least)
  if (!lanes_ok || apart[0] < 5 || apart[1] < 5 || apart[2] < 5 || apart[3] < 5 || split_apart < 5) ++fails;

  real *d_in = nullptr, *d_out = nullptr;
  std::vector<real> got(N_OUT);
  HIP_OK(hipMalloc(&d_in, in.size() * sizeof(real)));
  HIP_OK(hipMalloc(&d_out, N_OUT * sizeof(real)));
  HIP_OK(hipMemcpy(d_in, in.data(), in.size() * sizeof(real), hipMemcpyHostToDevice));
  HIP_OK(hipMemset(d_out, 0xff, N_OUT * sizeof(real)));
  hipLaunchKernelGGL(reduce_kernel<real>, dim3(1), dim3(64), 0, 0, d_in, d_out);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(got.data(), d_out, N_OUT * sizeof(real), hipMemcpyDeviceToHost));
  HIP_OK(hipFree(d_in));
  HIP_OK(hipFree(d_out));

  const struct { const char* what; int n; } groups[] = {{"wave_sum", SUM_SETS}, {"wave_max", MAX_SETS}, {"wave_min", MAX_SETS}, {"wave_sum_n<2>", 2},
                                                        {"wave_sum_n<3>", 3}, {"wave_sum_split<7>", 7}, {"wave_sum_split<32>", 32}};
  o = 0;
  for (const auto& g : groups) {
    int bad = 0;
    for (int k = 0; k < g.n; ++k, ++o)
      if (!same_bits(got[o], want[o])) {
        if (!bad++) std::printf("%s %s[%d]: device %.17g, host %.17g\n", name, g.what, k, (double)got[o], (double)want[o]);
      }
    std::printf("%s %s: %d of %d bit-equal\n", name, g.what, g.n - bad, g.n);
    fails += bad != 0;
  }
  return fails;
}

}  // namespace

int main() {
  const int fails = run<double>("double") + run<float>("float");
  std::printf(fails ? "FAIL\n" : "PASS\n");
  return fails ? 1 : 0;
}
