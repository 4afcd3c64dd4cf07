// check.cpp -- csrc/lmpc_fleet_reg_kernel.hip and csrc/lmpc_reg_kernel.hip compiled for the HOST (hip/hip_runtime.h in this directory stands in for the runtime)
// and run one thread at a time on a hand-built fleet store, before the kernels are ever launched on a device.  Built with
// -fsanitize=address,undefined, so an out-of-bounds row index is a crash here.  check.py writes the cases, runs this program and
// holds its output to oracle.regression; see there for the build line.
//
//   in:  B R C N, the spec, the vehicle, then `phases` states of the fleet (per car: changed?, its closed laps oldest first) and the
//        queries with the arrays the result is added onto
//   out: A, Bm, g after each phase (the arrays of lmpc_linearize_batch)
// Checked here, beside the bounds: the workspace layout against the array layout bit for bit; a car whose lap_count did not move is
// NOT packed again (a sentinel left in its table survives) unless every stamp was invalidated; counters of a store that hold garbage
// (head, cnt, npts, nrow out of range) read and write nothing outside the car's slots and table; the shared-store kernels of
// lmpc_reg_kernel.hip (residual, pack, lmpc_regress_kernel) on each car's laps in turn, sized as lmpc_set_regression_laps sizes them:
// the EXACT instances return the fleet kernel's bits for that car's queries (one core, the same rows in the same order), the
// expanded-distance instances agree to the oracle's bound.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define LMPC_FLEET_REG_NO_LAUNCHER
#include "lmpc_fleet_reg_kernel.hip"
#include "lmpc_reg_kernel.hip"

dim3 blockIdx, threadIdx, blockDim;

static FILE* fin;
static int rd_i() {
  int v;
  if (fread(&v, sizeof v, 1, fin) != 1) abort();
  return v;
}
static void rd_d(double* p, size_t n) {
  if (n && fread(p, sizeof(double), n, fin) != n) abort();
}

struct Store {
  lmpc_fleet_store st;
  std::vector<double2> key;
  std::vector<double> xr, aux, metad;
  std::vector<int> meta;
  Store(int B, int R, int C) {
    const size_t slots = (size_t)B * (R + 1), rows = slots * C;
    key.assign(rows, double2{NAN, NAN});  // what no closed lap holds is NaN: reading it shows in the result
    xr.assign(rows * 4, NAN);
    aux.assign(rows * 4, NAN);
    meta.assign(slots + 7 * (size_t)B, 0);
    metad.assign((size_t)B * (1 + LMPC_FLEET_DUR), 0.0);
    st.B = B, st.R = R, st.C = C;
    st.key = key.data(), st.xr = xr.data(), st.aux = aux.data();
    st.npts = meta.data();
    st.head = st.npts + slots;
    st.cnt = st.head + B;
    st.open_n = st.cnt + B;
    st.flags = st.open_n + B;
    st.lap_count = st.flags + B;
    st.n_dropped = st.lap_count + B;
    st.dur_n = st.n_dropped + B;
    st.s_prev = metad.data();
    st.dur = st.s_prev + B;
  }
};

static void run_pack(const Store& s, const lmpc_vehicle& veh, const lmpc_regression_spec& spec, int cap, double* tab, int* nrow, int* stamp,
                     unsigned threads) {
  blockDim = dim3(threads);
  for (unsigned b = 0; b < (unsigned)s.st.B; ++b)
    for (int t = (int)threads - 1; t >= 0; --t) {
      blockIdx = dim3(b), threadIdx = dim3((unsigned)t);
      lmpc_fleet_reg_pack_kernel(s.st, veh, spec, cap, tab, nrow, stamp);
    }
}

template <bool WS>
static void run_regress(int N, int B, const lmpc_regression_spec& spec, int cap, const double* tab, const int* nrow, const double* X, const double* U,
                        double* A, double* Bm, double* g) {
  const int chunks = (N - 1 + 63) / 64;
  const bool five = spec.n_in_state + spec.n_in_ctrl == 5;
  blockDim = dim3(64);
  for (unsigned blk = 0; blk < (unsigned)(B * chunks); ++blk)
    for (unsigned t = 0; t < 64; ++t) {
      blockIdx = dim3(blk), threadIdx = dim3(t);
      if (five)
        lmpc_fleet_regress_kernel<5, 3, WS>(N, B, chunks, spec, cap, tab, nrow, X, U, A, Bm, g);
      else
        lmpc_fleet_regress_kernel<8, 6, WS>(N, B, chunks, spec, cap, tab, nrow, X, U, A, Bm, g);
    }
}

// The shared-store path on car c's closed laps (oldest first, as its table has them; a lap of one sample is refused by
// lmpc_set_regression_laps and adds nothing to the car's table): every query of the batch runs against the table, car c's own
// queries are held to what the fleet kernel left in (A, Bm, g).  Returns the number of findings.
template <int NF, int NOUT>
static int run_shared(const Store& s, int c, const lmpc_vehicle& veh, const lmpc_regression_spec& spec, int N, const double* X, const double* U,
                      const std::vector<double>& A0, const std::vector<double>& B0, const std::vector<double>& g0, const std::vector<double>& A,
                      const std::vector<double>& Bm, const std::vector<double>& g) {
  const int B = s.st.B, R1 = s.st.R + 1, C = s.st.C, NS = N - 1, cnt = s.st.cnt[c], head = s.st.head[c];
  std::vector<double> x, u, k, t;
  std::vector<int> end, valid;
  for (int a = 0; a < cnt; ++a) {
    const int sl = ((head - cnt + a) % R1 + R1) % R1, n = s.st.npts[(size_t)c * R1 + sl];
    if (n < 2) continue;
    const size_t r0 = ((size_t)c * R1 + sl) * C;
    for (int j = 0; j < n; ++j) {
      x.push_back(s.key[r0 + j].x), x.push_back(s.key[r0 + j].y);
      for (int q = 0; q < 4; ++q) x.push_back(s.xr[(r0 + j) * 4 + q]);
      u.push_back(s.aux[(r0 + j) * 4]), u.push_back(s.aux[(r0 + j) * 4 + 1]);
      k.push_back(s.aux[(r0 + j) * 4 + 2]), t.push_back(s.aux[(r0 + j) * 4 + 3]);
      if (j + 1 < n) valid.push_back((int)end.size());
      end.push_back(j + 1 == n);
    }
  }
  const int total = (int)end.size(), nvalid = (int)valid.size(), npad = (nvalid + 3) / 4 * 4;
  if (!total) return 0;
  std::vector<double> y((size_t)total * 6, NAN), tab((size_t)npad * (NF + NOUT + 1), NAN);
  double* zz = tab.data() + (size_t)npad * (NF + NOUT);
  blockDim = dim3(256);
  for (int j = 0; j < (total + 255) / 256 * 256; ++j) {
    blockIdx = dim3((unsigned)j / 256), threadIdx = dim3((unsigned)j % 256);
    lmpc_reg_residual_kernel(veh, total, spec.as_written, end.data(), x.data(), u.data(), k.data(), t.data(), y.data());
  }
  for (int v = 0; v < (npad + 255) / 256 * 256; ++v) {
    blockIdx = dim3((unsigned)v / 256), threadIdx = dim3((unsigned)v % 256);
    lmpc_reg_pack_kernel(spec, nvalid, npad, valid.data(), x.data(), u.data(), y.data(), tab.data(), zz);
  }
  int bad = 0;
  blockDim = dim3(64);
  const unsigned blocks = (unsigned)((B * NS + 63) / 64);
  for (int exact = 1; exact >= 0; --exact) {
    std::vector<double> As(A0), Bs(B0), gs(g0), ws((size_t)B * NS * LMPC_LIN_RECORD, 0.0);
    for (unsigned blk = 0; blk < blocks; ++blk)
      for (unsigned th = 0; th < 64; ++th) {
        blockIdx = dim3(blk), threadIdx = dim3(th);
        if (exact) {
          lmpc_regress_kernel<NF, NOUT, false, true>(N, B, spec, npad, tab.data(), zz, X, U, As.data(), Bs.data(), gs.data());
          lmpc_regress_kernel<NF, NOUT, true, true>(N, B, spec, npad, tab.data(), zz, X, U, ws.data(), nullptr, nullptr);
        } else {
          lmpc_regress_kernel<NF, NOUT, false, false>(N, B, spec, npad, tab.data(), zz, X, U, As.data(), Bs.data(), gs.data());
          lmpc_regress_kernel<NF, NOUT, true, false>(N, B, spec, npad, tab.data(), zz, X, U, ws.data(), nullptr, nullptr);
        }
      }
    // car c's queries: the array layout against the fleet kernel's result, the record (started from zero) against its increment
    double scale = 1.0;
    for (int pass = 0; pass < 2; ++pass)
      for (int i = 0; i < NS; ++i) {
        const double* rec = &ws[((size_t)c * NS + i) * LMPC_LIN_RECORD];
        for (int e = 0; e < 54; ++e) {
          const int col = e / 6, r = e % 6;  // e < 48: [A B] column col, row r; then g
          const size_t o = e >= 48 ? ((size_t)(e - 48) * NS + i) * B + c
                                   : (col < 6 ? ((size_t)(r * 6 + col) * NS + i) * B + c : ((size_t)(r * 2 + col - 6) * NS + i) * B + c);
          const double got = e >= 48 ? gs[o] : (col < 6 ? As[o] : Bs[o]), ref = e >= 48 ? g[o] : (col < 6 ? A[o] : Bm[o]);
          const double was = e >= 48 ? g0[o] : (col < 6 ? A0[o] : B0[o]);
          if (!pass) {
            scale = std::fmax(scale, 1.0 + std::fabs(ref));
            continue;
          }
          if (exact ? memcmp(&got, &ref, 8) != 0 : !(std::fabs(got - ref) <= 1e-9 * scale)) ++bad;
          if (!(std::fabs(was + rec[e] - got) <= 1e-12 * scale)) ++bad;
        }
      }
  }
  if (bad) fprintf(stderr, "shared kernels on car %d's laps: %d findings\n", c, bad);
  return bad;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  fin = fopen(argv[1], "rb");
  FILE* fout = fopen(argv[2], "wb");
  if (!fin || !fout) return 2;
  const int B = rd_i(), R = rd_i(), C = rd_i(), N = rd_i(), NS = N - 1;
  lmpc_regression_spec spec{};
  spec.n_in_state = rd_i(), spec.n_in_ctrl = rd_i(), spec.n_out = rd_i();
  for (int& v : spec.in_state) v = rd_i();
  for (int& v : spec.in_ctrl) v = rd_i();
  for (int& v : spec.out) v = rd_i();
  spec.as_written = rd_i();
  const int phases = rd_i();
  rd_d(&spec.dist_max, 1);
  lmpc_vehicle veh;
  if (fread(&veh, sizeof veh, 1, fin) != 1) abort();
  const int nf = spec.n_in_state + spec.n_in_ctrl, stride = nf + spec.n_out + 1, cap = lmpc_fleet_reg_cap(R, C), R1 = R + 1;
  Store s(B, R, C);
  // exactly the sizes lmpc_fleet_ss_set_regression allocates: one row too far is the sanitizer's
  std::vector<double> tab((size_t)B * cap * stride, NAN);
  std::vector<int> nrow((size_t)B, 0), stamp((size_t)B, LMPC_FLEET_REG_STALE);
  const size_t nX = (size_t)6 * N * B, nU = (size_t)2 * NS * B, nA = (size_t)36 * NS * B, nB = (size_t)12 * NS * B, nG = (size_t)6 * NS * B;
  std::vector<double> X(nX), U(nU), A0(nA), B0(nB), g0(nG);
  int bad = 0;
  for (int p = 0; p < phases; ++p) {
    const int invalidate = rd_i();
    std::vector<int> changed((size_t)B);
    for (int b = 0; b < B; ++b) {
      changed[b] = rd_i();
      const int nl = rd_i();
      if (!changed[b] && nl != -1) abort();
      if (!changed[b]) continue;
      // the car's ring written anew at another rotation; the open lap's slot and every unused slot hold NaN and a wild npts
      const int head = (b + 2 * p + 1) % R1;
      for (int sl = 0; sl < R1; ++sl) {
        const size_t r0 = ((size_t)b * R1 + sl) * C;
        for (int j = 0; j < C; ++j) {
          s.key[r0 + j] = double2{NAN, NAN};
          for (int c = 0; c < 4; ++c) s.xr[(r0 + j) * 4 + c] = s.aux[(r0 + j) * 4 + c] = NAN;
        }
        s.st.npts[(size_t)b * R1 + sl] = C + 7;
      }
      if (nl > R) abort();
      for (int a = 0; a < nl; ++a) {
        const int sl = ((head - nl + a) % R1 + R1) % R1, n = rd_i();
        if (n < 1 || n > C) abort();
        std::vector<double> x((size_t)n * 6), u((size_t)n * 2), k((size_t)n), t((size_t)n);
        rd_d(x.data(), x.size()), rd_d(u.data(), u.size()), rd_d(k.data(), k.size()), rd_d(t.data(), t.size());
        const size_t r0 = ((size_t)b * R1 + sl) * C;
        for (int j = 0; j < n; ++j) {
          s.key[r0 + j] = double2{x[(size_t)j * 6], x[(size_t)j * 6 + 1]};
          for (int c = 0; c < 4; ++c) s.xr[(r0 + j) * 4 + c] = x[(size_t)j * 6 + 2 + c];
          s.aux[(r0 + j) * 4] = u[(size_t)j * 2], s.aux[(r0 + j) * 4 + 1] = u[(size_t)j * 2 + 1];
          s.aux[(r0 + j) * 4 + 2] = k[j], s.aux[(r0 + j) * 4 + 3] = t[j];
        }
        s.st.npts[(size_t)b * R1 + sl] = n;
      }
      s.st.head[b] = head, s.st.cnt[b] = nl, s.st.open_n[b] = 3;
      if (!invalidate) s.st.lap_count[b] += 1 + (b % 3);  // (an invalidated phase keeps the count: a reset and a load of as many laps)
    }
    if (invalidate)
      for (int& v : stamp) v = LMPC_FLEET_REG_STALE;
    rd_d(X.data(), nX), rd_d(U.data(), nU), rd_d(A0.data(), nA), rd_d(B0.data(), nB), rd_d(g0.data(), nG);
    // a sentinel in the table of every car that must not be packed again (first row, first residual: no query's distance reads it)
    std::vector<double> kept((size_t)B, 0.0);
    for (int b = 0; b < B; ++b)
      if (p > 0 && !invalidate && !changed[b] && nrow[b] > 0) {
        double& cell = tab[(size_t)b * cap * stride + nf];
        kept[b] = cell;
        cell = -12345.678;
      }
    run_pack(s, veh, spec, cap, tab.data(), nrow.data(), stamp.data(), p % 2 ? 64u : 256u);
    for (int b = 0; b < B; ++b) {
      if (p > 0 && !invalidate && !changed[b] && nrow[b] > 0) {
        double& cell = tab[(size_t)b * cap * stride + nf];
        if (cell != -12345.678) ++bad, fprintf(stderr, "phase %d car %d: packed again although its lap_count stood still\n", p, b);
        cell = kept[b];
      }
      if (stamp[b] != s.st.lap_count[b]) ++bad, fprintf(stderr, "phase %d car %d: stamp %d, lap_count %d\n", p, b, stamp[b], s.st.lap_count[b]);
      if (nrow[b] % 4 || nrow[b] < 0 || nrow[b] > cap) ++bad, fprintf(stderr, "phase %d car %d: nrow %d\n", p, b, nrow[b]);
    }
    std::vector<double> A(A0), Bm(B0), g(g0), ws((size_t)B * NS * LMPC_LIN_RECORD);
    for (int b = 0; b < B; ++b)
      for (int i = 0; i < NS; ++i) {
        double* rec = &ws[((size_t)b * NS + i) * LMPC_LIN_RECORD];
        for (int col = 0; col < 8; ++col)
          for (int r = 0; r < 6; ++r)
            rec[col * 6 + r] = col < 6 ? A0[((size_t)(r * 6 + col) * NS + i) * B + b] : B0[((size_t)(r * 2 + col - 6) * NS + i) * B + b];
        for (int r = 0; r < 6; ++r) rec[48 + r] = g0[((size_t)r * NS + i) * B + b];
      }
    run_regress<false>(N, B, spec, cap, tab.data(), nrow.data(), X.data(), U.data(), A.data(), Bm.data(), g.data());
    run_regress<true>(N, B, spec, cap, tab.data(), nrow.data(), X.data(), U.data(), ws.data(), nullptr, nullptr);
    for (int b = 0; b < B; ++b)
      for (int i = 0; i < NS; ++i) {
        const double* rec = &ws[((size_t)b * NS + i) * LMPC_LIN_RECORD];
        for (int col = 0; col < 8; ++col)
          for (int r = 0; r < 6; ++r) {
            const double a = col < 6 ? A[((size_t)(r * 6 + col) * NS + i) * B + b] : Bm[((size_t)(r * 2 + col - 6) * NS + i) * B + b];
            if (memcmp(&a, &rec[col * 6 + r], 8)) ++bad;
          }
        for (int r = 0; r < 6; ++r)
          if (memcmp(&g[((size_t)r * NS + i) * B + b], &rec[48 + r], 8)) ++bad;
      }
    for (int c = 0; c < B; ++c)
      bad += nf == 5 ? run_shared<5, 3>(s, c, veh, spec, N, X.data(), U.data(), A0, B0, g0, A, Bm, g)
                     : run_shared<8, 6>(s, c, veh, spec, N, X.data(), U.data(), A0, B0, g0, A, Bm, g);
    fwrite(A.data(), 8, nA, fout), fwrite(Bm.data(), 8, nB, fout), fwrite(g.data(), 8, nG, fout);
  }
  // garbage in every counter: nothing outside the slots is read, nothing outside the table written (the sanitizer's to say)
  for (int b = 0; b < B; ++b) {
    s.st.head[b] = b % 2 ? -7 : 1000000;
    s.st.cnt[b] = b % 3 ? 1 << 30 : -5;
    for (int sl = 0; sl < R1; ++sl) s.st.npts[(size_t)b * R1 + sl] = (b + sl) % 2 ? 2000000000 : -3;
    s.st.lap_count[b] += 1;
  }
  run_pack(s, veh, spec, cap, tab.data(), nrow.data(), stamp.data(), 256u);
  for (int b = 0; b < B; ++b) nrow[b] = b % 2 ? 2000000001 : -9;
  {
    std::vector<double> A(A0), Bm(B0), g(g0);
    run_regress<false>(N, B, spec, cap, tab.data(), nrow.data(), X.data(), U.data(), A.data(), Bm.data(), g.data());
  }
  fclose(fout);
  if (bad) fprintf(stderr, "%d findings\n", bad);
  printf("host check: %d phases, B %d R %d C %d N %d (%d, %d): %s\n", phases, B, R, C, N, nf, spec.n_out, bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
