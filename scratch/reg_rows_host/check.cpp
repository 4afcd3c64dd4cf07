// check.cpp -- csrc/lmpc_reg_rows_kernel.hip and csrc/lmpc_fleet_reg_rows_kernel.hip compiled for the HOST (scratch/fleet_reg_host/hip/hip_runtime.h
// stands in for the runtime) and run one thread at a time, before the kernels are ever launched on a device.  Built with
// -fsanitize=address,undefined, so an out-of-bounds row index is a crash here:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iscratch/fleet_reg_host -Iinclude \
//       -Iracing-lmpc-ros2_amd/csrc -x c++ scratch/reg_rows_host/check.cpp -o /tmp/reg_rows_check && /tmp/reg_rows_check
// Shared store: five specs (4 and 5 features per row, 1 .. 3 rows, lists of different lengths, rows out of order), both signs, tables of
// 1, 37 and 64 samples, both output layouts, against a dense solve of each row's own normal equations at 1e-9; entries outside a touched
// row's lists must keep their bits.  Per car: a store whose counters hold garbage (cnt 99, head -5, npts 1000, nrow 2^30) reads and
// writes nothing outside the car's slots and table.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <random>
#define LMPC_FLEET_REG_NO_LAUNCHER
#include "lmpc_fleet_reg_kernel.hip"
#include "lmpc_reg_rows_kernel.hip"
dim3 blockIdx, threadIdx, blockDim;

static void solve_dense(int n, std::vector<double> Q, std::vector<double> b, double* R) {
  for (int c = 0; c < n; ++c) {
    int p = c;
    for (int r = c + 1; r < n; ++r) if (fabs(Q[r*n+c]) > fabs(Q[p*n+c])) p = r;
    for (int k = 0; k < n; ++k) std::swap(Q[c*n+k], Q[p*n+k]);
    std::swap(b[c], b[p]);
    for (int r = c + 1; r < n; ++r) { double f = Q[r*n+c]/Q[c*n+c]; for (int k = c; k < n; ++k) Q[r*n+k] -= f*Q[c*n+k]; b[r] -= f*b[c]; }
  }
  for (int r = n-1; r >= 0; --r) { double t = b[r]; for (int k = r+1; k < n; ++k) t -= Q[r*n+k]*R[k]; R[r] = t/Q[r*n+r]; }
}

struct Store {
  lmpc_fleet_store st;
  std::vector<double2> key; std::vector<double> xr, aux, metad; std::vector<int> meta;
  Store(int B, int R, int C) {
    const size_t slots = (size_t)B * (R + 1), rows = slots * C;
    key.assign(rows, double2{NAN, NAN}); xr.assign(rows * 4, NAN); aux.assign(rows * 4, NAN);
    meta.assign(slots + 7 * (size_t)B, 0); metad.assign((size_t)B * (1 + LMPC_FLEET_DUR), 0.0);
    st.B = B, st.R = R, st.C = C; st.key = key.data(), st.xr = xr.data(), st.aux = aux.data();
    st.npts = meta.data(); st.head = st.npts + slots; st.cnt = st.head + B; st.open_n = st.cnt + B; st.flags = st.open_n + B;
    st.lap_count = st.flags + B; st.n_dropped = st.lap_count + B; st.dur_n = st.n_dropped + B; st.s_prev = metad.data(); st.dur = st.s_prev + B;
  }
};

int main() {
  std::mt19937_64 rng(7);
  std::normal_distribution<double> nd(0, 1);
  int bad = 0;
  struct Case { int n_out; int out[3]; int ns[3]; int is[3][6]; int nc[3]; int ic[3][2]; };
  Case cases[] = {
    {3, {3,4,5}, {3,3,3}, {{3,4,5},{3,4,5},{3,4,5}}, {1,1,1}, {{0},{1},{1}}},
    {3, {3,4,5}, {1,3,4}, {{3},{3,4,5},{2,3,4,5}}, {1,1,1}, {{0},{1},{1}}},
    {2, {5,3}, {3,2}, {{3,4,5},{4,3}}, {2,0}, {{1,0},{0}}},
    {1, {4}, {1}, {{4}}, {0}, {{0}}},
    {3, {0,1,2}, {5,3,3}, {{0,1,2,3,4},{3,4,5},{3,4,5}}, {0,2,2}, {{0},{0,1},{1,0}}},
  };
  for (auto& cs : cases) for (int aw = 0; aw < 2; ++aw) for (int nval : {1, 37, 64}) {
    lmpc_regression_rows_spec sp{};
    sp.n_out = cs.n_out; sp.as_written = aw; sp.dist_max = 1.3;
    for (int o = 0; o < cs.n_out; ++o) { sp.out[o] = cs.out[o]; sp.n_in_state[o] = cs.ns[o]; sp.n_in_ctrl[o] = cs.nc[o];
      for (int f = 0; f < cs.ns[o]; ++f) sp.in_state[o][f] = cs.is[o][f]; for (int f = 0; f < cs.nc[o]; ++f) sp.in_ctrl[o][f] = cs.ic[o][f]; }
    lmpc_reg_rows_dev d; const char* msg = nullptr;
    if (lmpc_reg_rows_digest(&sp, &d, &msg)) { printf("digest refused: %s\n", msg); return 1; }
    const int N = 4, B = 23, NS = N - 1, nq = B * NS;
    const int npad = (nval + 3) / 4 * 4, stride = lmpc_reg_rows_stride(d);
    std::vector<double> x(nval*6), u(nval*2), y(nval*6), tab((size_t)npad*stride, NAN);
    std::vector<int> valid(nval);
    for (int j = 0; j < nval; ++j) valid[j] = j;
    for (auto& v : x) v = 0.5*nd(rng); for (auto& v : u) v = 0.5*nd(rng); for (auto& v : y) v = nd(rng);
    blockDim = dim3(256);
    for (int v = 0; v < 256; ++v) { blockIdx = dim3(0); threadIdx = dim3(v); lmpc_reg_rows_pack_kernel(d, nval, npad, valid.data(), x.data(), u.data(), y.data(), tab.data()); }
    std::vector<double> X(6*N*B), U(2*NS*B), A0(36*NS*B), B0(12*NS*B), g0(6*NS*B), W0((size_t)B*NS*54);
    for (auto& v : X) v = 0.5*nd(rng); for (auto& v : U) v = 0.5*nd(rng);
    // one query far from everything in row-2-only features
    for (auto* a : {&A0, &B0, &g0, &W0}) for (auto& v : *a) v = nd(rng);
    auto A = A0, Bm = B0, g = g0, W = W0;
    blockDim = dim3(64);
    for (unsigned blk = 0; blk < (unsigned)((nq + 63) / 64); ++blk) for (unsigned t = 0; t < 64; ++t) {
      blockIdx = dim3(blk); threadIdx = dim3(t);
      if (d.mf == 4) { lmpc_regress_rows_kernel<4, false>(N, B, d, npad, tab.data(), X.data(), U.data(), A.data(), Bm.data(), g.data());
                       lmpc_regress_rows_kernel<4, true>(N, B, d, npad, tab.data(), X.data(), U.data(), W.data(), nullptr, nullptr); }
      else { lmpc_regress_rows_kernel<5, false>(N, B, d, npad, tab.data(), X.data(), U.data(), A.data(), Bm.data(), g.data());
             lmpc_regress_rows_kernel<5, true>(N, B, d, npad, tab.data(), X.data(), U.data(), W.data(), nullptr, nullptr); }
    }
    // reference
    auto Ar = A0, Br = B0, gr = g0, Wr = W0;
    int touched = 0, untouched = 0;
    for (int b = 0; b < B; ++b) for (int i = 0; i < NS; ++i) for (int o = 0; o < cs.n_out; ++o) {
      const int nf = d.nf[o], nm = nf + 1;
      std::vector<double> q(nf), Q(nm*nm, 0.0), rhs(nm, 0.0);
      for (int f = 0; f < nf; ++f) { int c = d.col[o][f]; q[f] = c < 6 ? X[((size_t)c*N+i)*B+b] : U[((size_t)(c-6)*NS+i)*B+b]; }
      bool any = false;
      for (int j = 0; j < nval; ++j) {
        std::vector<double> m(nm, 1.0); double d2 = 0;
        for (int f = 0; f < nf; ++f) { int c = d.col[o][f]; m[f] = c < 6 ? x[j*6+c] : u[j*2+c-6]; d2 += (m[f]-q[f])*(m[f]-q[f]); }
        if (!(sqrt(d2) < sp.dist_max)) continue;
        any = true;
        double K = 0.75/sp.dist_max * pow(1 - d2/(sp.dist_max*sp.dist_max), 2);
        for (int r = 0; r < nm; ++r) { for (int c = 0; c < nm; ++c) Q[r*nm+c] += K*m[r]*m[c]; rhs[r] += (aw ? -1 : 1)*K*m[r]*y[j*6+d.out[o]]; }
      }
      if (!any) { ++untouched; continue; }
      ++touched;
      for (int r = 0; r < nm; ++r) Q[r*nm+r] += 1e-3;
      std::vector<double> R(nm);
      solve_dense(nm, Q, rhs, R.data());
      const int ro = d.out[o];
      for (int f = 0; f < nf; ++f) { int c = d.col[o][f];
        if (c < 6) Ar[((size_t)(ro*6+c)*NS+i)*B+b] += R[f]; else Br[((size_t)(ro*2+c-6)*NS+i)*B+b] += R[f];
        Wr[((size_t)b*NS+i)*54 + c*6 + ro] += R[f]; }
      gr[((size_t)ro*NS+i)*B+b] += R[nf]; Wr[((size_t)b*NS+i)*54 + 48 + ro] += R[nf];
    }
    double e = 0; size_t nchg = 0, nsame = 0;
    auto cmp = [&](const std::vector<double>& a, const std::vector<double>& r, const std::vector<double>& z) {
      for (size_t k = 0; k < a.size(); ++k) { e = fmax(e, fabs(a[k]-r[k])/(1+fabs(r[k])));
        if (r[k] == z[k]) { if (memcmp(&a[k], &z[k], 8)) { ++bad; } else ++nsame; } else ++nchg; } };
    cmp(A, Ar, A0); cmp(Bm, Br, B0); cmp(g, gr, g0); cmp(W, Wr, W0);
    printf("n_out %d mf %d aw %d nval %d: touched %d untouched %d changed %zu same %zu err %.2e bad %d\n", cs.n_out, d.mf, aw, nval, touched, untouched, nchg, nsame, e, bad);
    if (!(e < 1e-9)) ++bad;
  }
  // fleet: bounds only (garbage counters), and a pack + regress round on a small store with a zeroed vehicle
  {
    const int B = 3, R = 2, C = 9, N = 70;
    Store s(B, R, C);
    for (size_t r = 0; r < s.key.size(); ++r) { s.key[r] = double2{nd(rng), nd(rng)}; for (int c = 0; c < 4; ++c) { s.xr[r*4+c] = nd(rng); s.aux[r*4+c] = 0.1*nd(rng); } }
    int cnts[3] = {0, 1, 99}, heads[3] = {0, 1, -5};
    for (int b = 0; b < B; ++b) { s.st.cnt[b] = cnts[b]; s.st.head[b] = heads[b]; s.st.lap_count[b] = b + 1; for (int sl = 0; sl <= R; ++sl) s.st.npts[b*(R+1)+sl] = b == 2 ? 1000 : (sl ? 5 : 1); }
    lmpc_regression_rows_spec sp{}; sp.n_out = 3; sp.dist_max = 5.0;
    for (int o = 0; o < 3; ++o) { sp.out[o] = 3+o; sp.n_in_state[o] = 3; sp.n_in_ctrl[o] = 2; for (int f = 0; f < 3; ++f) sp.in_state[o][f] = 3+f; sp.in_ctrl[o][0] = 0; sp.in_ctrl[o][1] = 1; }
    lmpc_reg_rows_dev d; const char* msg;
    if (lmpc_reg_rows_digest(&sp, &d, &msg)) return 1;
    const int cap = lmpc_fleet_reg_cap(R, C), stride = lmpc_reg_rows_stride(d);
    std::vector<double> tab((size_t)B*cap*stride, NAN); std::vector<int> nrow(B, 0), stamp(B, -1);
    lmpc_vehicle veh{};
    blockDim = dim3(256);
    for (unsigned b = 0; b < (unsigned)B; ++b) for (int t = 255; t >= 0; --t) { blockIdx = dim3(b); threadIdx = dim3((unsigned)t); lmpc_fleet_reg_rows_pack_kernel(s.st, veh, d, cap, tab.data(), nrow.data(), stamp.data()); }
    printf("fleet nrow %d %d %d cap %d stamp %d %d %d\n", nrow[0], nrow[1], nrow[2], cap, stamp[0], stamp[1], stamp[2]);
    nrow[2] = 1 << 30;  // garbage
    const int NS = N - 1, chunks = (NS + 63) / 64;
    std::vector<double> X(6*N*B, 0.3), U(2*NS*B, 0.0), A(36*NS*B, 0), Bm(12*NS*B, 0), g(6*NS*B, 0), W((size_t)B*NS*54, 0);
    blockDim = dim3(64);
    for (unsigned blk = 0; blk < (unsigned)(B*chunks); ++blk) for (unsigned t = 0; t < 64; ++t) { blockIdx = dim3(blk); threadIdx = dim3(t);
      lmpc_fleet_regress_rows_kernel<5, false>(N, B, chunks, d, cap, tab.data(), nrow.data(), X.data(), U.data(), A.data(), Bm.data(), g.data());
      lmpc_fleet_regress_rows_kernel<5, true>(N, B, chunks, d, cap, tab.data(), nrow.data(), X.data(), U.data(), W.data(), nullptr, nullptr); }
    printf("fleet regress ran\n");
  }
  printf(bad ? "FAIL %d\n" : "OK %d\n", bad);
  return bad != 0;
}
