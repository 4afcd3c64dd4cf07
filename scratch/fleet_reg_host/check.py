"""The regression kernels (per car, and the shared-store ones) on the CPU, before any launch: writes the cases, runs ./check (check.cpp: the kernel file compiled for
the host, address and undefined-behaviour sanitizers on) and holds what it returns to oracle.regression at the GPU test's bound,
1e-9 (1 + max|ref|), untouched queries bit-identical.  From the repository root:

  g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iscratch/fleet_reg_host -Iinclude \
      -Iracing-lmpc-ros2_amd/csrc -x c++ scratch/fleet_reg_host/check.cpp -o /tmp/fleet_reg_check
  python scratch/fleet_reg_host/check.py /tmp/fleet_reg_check

Phases of one store (R = 3, C = 24): (0) every car loaded -- paddings 0..3, a car without a lap, one-sample and two-sample laps, full
rings; (1) every other car gets a new ring and a moved lap_count, the rest must not be packed again and must return the same bits;
(2) every car gets other laps under the SAME lap_count with every stamp invalidated (a reset and a load of as many laps).
After each phase check.cpp also runs the shared-store kernels of lmpc_reg_kernel.hip (residual, pack, lmpc_regress_kernel<5, 3> or
<8, 6>, both layouts, EXACT and not) on every car's laps in turn and holds that car's queries to the per-car kernel's result: the
EXACT instances bit for bit, the others at 1e-9 (1 + max|ref|)."""
import ctypes as C
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import __graft_entry__ as G  # noqa: E402
from oracle import params as P, qp as Q, regression as R, scenario as S  # noqa: E402
from test_regression_oracle import synthetic_lap  # noqa: E402

pkg = G.load_package()
capi = pkg.capi


def laps_of(veh, b, phase, R_, Cc):
    rng = np.random.default_rng(1000 * phase + b)
    if phase == 0 and b == 1:
        return []
    n_laps = 1 + (b + phase) % R_
    laps = []
    for l in range(n_laps):
        n = int(rng.integers(6, Cc + 1))
        if b == 2 and l == 0:
            n = 2
        if b == 3 and l == 0:
            n = 1          # a lap of one sample has none with a successor
        if b == 4:
            n = Cc          # full slots, full ring
        laps.append(synthetic_lap(veh, n, int(rng.integers(1 << 30))))
    if b == 4:
        laps = [synthetic_lap(veh, Cc, 77 + phase + l) for l in range(R_)]
    return laps


def laps_near(X, U, tr, b, phase, R_, Cc):
    """Laps around car b's own reference (every feature of the (8, 6) spec within reach of its queries, the abscissa among them)."""
    rng = np.random.default_rng(2000 * phase + b)
    laps = []
    for l in range(1 + (b + phase) % R_):
        n = int(rng.integers(6, Cc + 1))
        idx = rng.integers(0, U.shape[1], n)
        x = X[:, idx, b].T + rng.normal(0, 1, (n, 6)) * 0.15   # spread over the bandwidth: tests/test_gpu_fleet_regression.py NEAR_NOISE
        u = U[:, idx, b].T + rng.normal(0, 1, (n, 2)) * 0.15
        laps.append((x, u, S.track_lookup(tr["curvature"], x[:, 0], tr["L"]), np.cumsum(rng.uniform(0.02, 0.04, n))))
    return laps


def case(exe, N, spec, as_written, h, Bn=11, R_=3, Cc=24, near=False):
    ins, inc, outs = spec
    veh, cfg = P.barc_vehicle(), P.barc_tracking_mpc(N)
    tr = pkg.workloads.synthetic_track("barc")
    u_lo, u_hi, _, _ = Q.effective_bounds(cfg, veh)
    x, u = pkg.workloads.sample_initial_states("barc", Bn, tr["L"], u_lo, u_hi, 31)
    inp = S.cold_start_inputs(cfg, veh, tr, x, u, 0.025)
    X, U = np.ascontiguousarray(inp["X_ref"], dtype=np.float64), np.ascontiguousarray(inp["U_ref"], dtype=np.float64)
    rng = np.random.default_rng(5)
    A0, B0, g0 = rng.normal(size=(6, 6, N - 1, Bn)), rng.normal(size=(6, 2, N - 1, Bn)), rng.normal(size=(6, N - 1, Bn))
    cv = capi._fill(capi.CVehicle(), pkg.presets.barc_vehicle())
    pad6 = lambda v, n: list(v) + [0] * (n - len(v))
    blob = struct.pack("<4i", Bn, R_, Cc, N) + struct.pack("<3i", len(ins), len(inc), len(outs))
    blob += struct.pack("<6i", *pad6(ins, 6)) + struct.pack("<2i", *pad6(inc, 2)) + struct.pack("<6i", *pad6(outs, 6))
    blob += struct.pack("<2i", int(as_written), 3) + struct.pack("<d", h) + bytes(cv)
    state, states = [None] * Bn, []
    for phase in range(3):
        blob += struct.pack("<i", 1 if phase == 2 else 0)
        for b in range(Bn):
            changed = phase != 1 or b % 2 == 0
            if not changed:
                blob += struct.pack("<2i", 0, -1)
                continue
            laps = laps_near(X, U, tr, b, phase, R_, Cc) if near else laps_of(veh, b, phase, R_, Cc)
            state[b] = laps
            blob += struct.pack("<2i", 1, len(laps))
            for (lx, lu, lk, lt) in laps:
                blob += struct.pack("<i", lx.shape[0]) + b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in (lx, lu, lk, lt))
        states.append(list(state))
        blob += b"".join(a.tobytes() for a in (X, U, A0, B0, g0))
    with tempfile.TemporaryDirectory() as d:
        fi, fo = Path(d) / "in.bin", Path(d) / "out.bin"
        fi.write_bytes(blob)
        r = subprocess.run([exe, str(fi), str(fo)], capture_output=True, text=True)
        print(r.stdout.strip(), r.stderr.strip()[-2000:])
        assert r.returncode == 0
        out = np.frombuffer(fo.read_bytes(), dtype=np.float64)
    flat = lambda a: np.ascontiguousarray(np.moveaxis(a, (-1, -2), (0, 1)).reshape(Bn * (N - 1), *a.shape[:-2]))
    nA, nB, nG = A0.size, B0.size, g0.size
    res = []
    for phase in range(3):
        o = out[phase * (nA + nB + nG):]
        A, Bm, g = o[:nA].reshape(A0.shape), o[nA:nA + nB].reshape(B0.shape), o[nA + nB:nA + nB + nG].reshape(g0.shape)
        res.append((A, Bm, g))
        worst, n_touched = 0.0, 0
        for b in range(Bn):
            sl = slice(b * (N - 1), (b + 1) * (N - 1))
            a0, b0, c0 = flat(A0)[sl], flat(B0)[sl], flat(g0)[sl]
            laps = [l for l in states[phase][b] if l[0].shape[0] >= 2]
            if laps:
                Ar, Br, gr, touched = R.regress_batch(veh, laps, ins, inc, outs, h, flat(X[:, :N - 1])[sl], flat(U)[sl], a0, b0, c0, as_written=as_written)
            else:
                Ar, Br, gr, touched = a0, b0, c0, np.zeros(N - 1, dtype=bool)
            ak, bk, gk = flat(A)[sl], flat(Bm)[sl], flat(g)[sl]
            for ref, got in ((Ar, ak), (Br, bk), (gr, gk)):
                e = np.abs(ref - got).reshape(N - 1, -1).max(axis=1) / (1 + np.abs(ref).reshape(N - 1, -1).max(axis=1))
                worst = max(worst, e.max())
                assert np.array_equal(ref[~touched], got[~touched]), (phase, b)
            n_touched += int(touched.sum())
        print("  phase %d: worst %.1e, %d of %d queries touched" % (phase, worst, n_touched, Bn * (N - 1)))
        assert worst < 1e-9 and n_touched >= Bn * (N - 1) // 10
    for b in range(1, Bn, 2):   # the cars phase 1 left alone: the same bits
        for k in range(3):
            assert np.array_equal(res[0][k][..., b], res[1][k][..., b]), b


if __name__ == "__main__":
    exe = sys.argv[1]
    BENCH, S1234, ALL = ((3, 4, 5), (0, 1), (3, 4, 5)), ((1, 2, 3, 4), (1,), (3, 4, 5)), ((0, 1, 2, 3, 4, 5), (0, 1), (0, 1, 2, 3, 4, 5))
    case(exe, 20, BENCH, False, 0.6)
    case(exe, 3, S1234, True, 0.6)
    case(exe, 81, ALL, False, 1.5, Bn=5, near=True)
    case(exe, 20, ALL, True, 0.6, Bn=7, near=True)
    case(exe, 70, BENCH, True, 0.6, Bn=6)
    print("all host cases ok")
