"""The batched extended Kalman filter on the device (lmpc_ekf_*) against the plain numpy restatement of tests/ekf_cases.py.

Tolerance 1e-10 on x, P and K (ekf_cases.TOL): 3e4 times the restatement's measured distance from its extended-precision twin on the
same scenario (tests/test_ekf_reference.py), room for FMA contraction and the device's sincos / atan, nine orders below a wrong term.
Every scenario stays where the filter is well conditioned: vx >= 1.5 m/s for the truth, updates 12.5 ms apart at most."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ekf_cases as EC
import track_cases as TC
from oracle import params as OP

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "racing-lmpc-ros2_amd" / "lib"

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver(pkg):
    return pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)


@pytest.fixture(scope="module")
def sc():
    return EC.scenario(257)


class Dev:
    """The device filter behind the restatement's interface: arrays [B, ...] in numpy on the outside."""

    def __init__(self, solver, cfg, B, observations, x=None, P=None, initialize=True):
        import torch
        self.s, self.B, self.torch = solver, B, torch
        solver.ekf_create(B, cfg["x0"], cfg["P0"], cfg["Q"], cfg["x_min"], cfg["x_max"])
        self.ids = [solver.ekf_register_observation(r) for r in observations]
        if x is not None or P is not None:
            solver.ekf_set_state(None if x is None else self.dev(x[:B]), None if P is None else self.dev(P[:B]))
        if initialize:
            solver.ekf_initialize(0)

    def dev(self, a):
        a = np.asarray(a, dtype=np.float64)
        return self.torch.as_tensor(np.ascontiguousarray(np.moveaxis(a, 0, -1)), device=self.s.device)

    @staticmethod
    def host(t):
        return None if t is None else np.moveaxis(t.cpu().numpy(), -1, 0)

    def update(self, obs, z, R, ns, u=None, out=None):
        if u is not None:
            self.s.ekf_update_control(self.dev(u[:self.B]))
        res = self.s.ekf_update(obs, None if z is None else self.dev(z[:self.B]), None if R is None else self.dev(R[:self.B]), ns, out=out)
        return tuple(self.host(t) for t in res)

    def get(self):
        g = self.s.ekf_get()
        return {k: (self.host(v) if k in ("x", "P", "K") else v) for k, v in g.items()}


def _scenario_filter(solver, sc, B):
    return Dev(solver, sc["cfg"], B, (EC.ROWS_VEL, EC.ROWS_POSE), sc["x0"], sc["P0"])


def _cmp(worst, got, ref):
    """max |difference| of x, P, Kz into worst[0:3]; flags must be equal."""
    for i in range(3):
        if ref[i] is not None:
            worst[i] = max(worst[i], float(np.abs(got[i] - ref[i]).max()))
    assert np.array_equal(got[3], ref[3]), (got[3], ref[3])


def test_parity_on_the_scenario(solver, sc):
    """B = 257 (one full 256-thread block and one lane of the next), 400 periods, both observations, 10 % pose dropouts: every estimate,
    covariance, Kz and flag after every update; lmpc_ekf_get returns the last outputs bit for bit."""
    B = 257
    dev, ref = _scenario_filter(solver, sc, B), EC.new_filter(sc)
    worst, n_drop = [0.0, 0.0, 0.0], 0
    for obs, z, R, u, ns in sc["updates"]:
        ref.update_control(u)
        want = ref.update(obs, z, R, ns)
        got = dev.update(obs, z, R, ns, u=u)
        _cmp(worst, got, want)
        n_drop += int((want[3] & EC.FALLBACK).sum())
    print("parity B = %d, %d updates, %d dropouts: |dx| %.2e |dP| %.2e |dKz| %.2e" % (B, len(sc["updates"]), n_drop, *worst))
    assert n_drop > 0.05 * 400 * B
    assert max(worst) <= EC.TOL, worst
    g = dev.get()
    assert np.array_equal(g["x"], got[0]) and np.array_equal(g["P"], got[1]) and np.array_equal(g["K"][:, :, 2:5], got[2])
    assert np.abs(g["K"] - ref.K).max() <= EC.TOL
    assert g["timestamp_ns"] == sc["updates"][-1][4] and g["initialized"]


def test_every_observation_size(solver, sc):
    """Observations of 1 .. 6 rows, one of them the permuted list (5, 2, 0), B = 64, 20 updates each, dense random SPD R per car."""
    B, rng = 64, np.random.default_rng(21)
    observations = ((0,), (3, 5), (5, 2, 0), (0, 1, 2, 3), (1, 2, 3, 4, 5), (0, 1, 2, 3, 4, 5))
    dev = Dev(solver, sc["cfg"], B, observations, sc["x0"], sc["P0"])
    ref = EC.Filter(sc["veh"], sc["cfg"], B)
    for r in observations:
        ref.register_observation(r)
    ref.set_state(sc["x0"][:B], sc["P0"][:B])
    ref.initialize(0)
    sig = np.array([0.02, 0.02, 0.01, 0.05, 0.05, 0.05])
    worst, ns, u = [0.0, 0.0, 0.0], 0, sc["updates"][0][3][:B]
    truth = sc["x0"][:B].copy()
    truth[:, 3] = np.maximum(truth[:, 3], 1.5)
    for k in range(20):
        for oid, rows in enumerate(observations):
            ns += 5_000_000
            truth = EC.D.rk4(truth, u, 0.0, 0.005, sc["veh"])
            z = truth[:, list(rows)] + rng.normal(0, 1, (B, len(rows))) * sig[list(rows)]
            if 2 in rows:
                j = rows.index(2)
                z[:, j] = np.arctan2(np.sin(z[:, j]), np.cos(z[:, j]))
            R = EC.spd(rng, B, len(rows))
            ref.update_control(u)
            _cmp(worst, dev.update(oid, z, R, ns, u=u), ref.update(oid, z, R, ns))
    print("nz = 1 .. 6, B = %d, 20 updates each: |dx| %.2e |dP| %.2e |dKz| %.2e" % (B, *worst))
    assert max(worst) <= EC.TOL, worst
    assert np.abs(dev.get()["K"] - ref.K).max() <= EC.TOL and ref.K.shape[2] == 21


def _warm(solver, sc, B=64):
    """A filter two updates into the scenario (a non-zero gain, a non-diagonal P), and the next pose update's clean inputs."""
    dev = _scenario_filter(solver, sc, B)
    for obs, z, R, u, ns in sc["updates"][:2]:
        dev.update(obs, z, R, ns, u=u)
    _, z, R, u, ns = sc["updates"][3]
    return dev, np.nan_to_num(z[:B], nan=0.2), R[:B].copy(), u, ns


def test_fallback_cars_take_the_prediction_and_leave_their_neighbours_alone(solver, sc):
    dev, z, R, u, ns = _warm(solver, sc)
    clean = dev.update(1, z, R, ns, u=u)
    k_clean = dev.get()["K"]
    dev, _, _, _, _ = _warm(solver, sc)
    again = dev.update(1, z, R, ns, u=u)
    assert all(np.array_equal(a, b) for a, b in zip(clean, again))          # reproducible across two runs
    dev, _, _, _, _ = _warm(solver, sc)
    k_before = dev.get()["K"]
    zd, Rd = z.copy(), R.copy()
    zd[3, 1] = np.nan
    Rd[5, 2, 0] = np.inf
    Rd[9, 1, 1] = -np.inf
    dirty = dev.update(1, zd, Rd, ns, u=u)
    k_dirty = dev.get()["K"]
    dev, _, _, _, _ = _warm(solver, sc)
    pred = dev.update(-1, None, None, ns, u=u)
    bad = np.zeros(64, dtype=bool)
    bad[[3, 5, 9]] = True
    assert np.array_equal(dirty[3], np.where(bad, EC.FALLBACK, 0)) and not clean[3].any() and not pred[3].any() and pred[2] is None
    for i in (0, 1):
        assert np.array_equal(dirty[i][bad], pred[i][bad]) and np.array_equal(dirty[i][~bad], clean[i][~bad])
    assert np.array_equal(k_dirty[bad], k_before[bad]) and np.array_equal(k_dirty[~bad], k_clean[~bad])
    assert np.array_equal(dirty[2][bad], k_before[bad][:, :, 2:5]) and np.array_equal(dirty[2][~bad], clean[2][~bad])


def test_null_outputs_and_batch_of_one(pkg, solver, sc):
    import torch
    dev, z, R, u, ns = _warm(solver, sc)
    full = dev.update(1, z, R, ns, u=u)
    g_full = dev.get()
    kw = dict(dtype=torch.float64, device=solver.device)
    for keep in ((0,), (1, 3), (2,), ()):
        dev, _, _, _, _ = _warm(solver, sc)
        bufs = [torch.empty((6, 64), **kw), torch.empty((6, 6, 64), **kw), torch.empty((6, 3, 64), **kw),
                torch.empty((64,), dtype=torch.int32, device=solver.device)]
        part = dev.update(1, z, R, ns, u=u, out=tuple(b if i in keep else None for i, b in enumerate(bufs)))
        for i in range(4):
            assert (part[i] is None) if i not in keep else np.array_equal(part[i], full[i]), (keep, i)
        g = dev.get()
        assert all(np.array_equal(g[k], g_full[k]) for k in ("x", "P", "K"))
    other = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)   # (a handle holds one filter)
    one = _scenario_filter(other, sc, 1)
    many = _scenario_filter(solver, sc, 64)
    for obs, zz, RR, uu, t in sc["updates"][:12]:
        a, b = one.update(obs, zz, RR, t, u=uu), many.update(obs, zz, RR, t, u=uu)
        assert all(np.array_equal(p[0], q[0]) for p, q in zip(a, b))        # B = 1 and B = 64 give the same car 0
    other.close()


def test_check_cov_and_a_backward_timestamp_match_the_restatement(solver, sc):
    B = 64
    dev, ref = _scenario_filter(solver, sc, B), EC.new_filter(sc, B=B)
    worst = [0.0, 0.0, 0.0]
    (_, zv, Rv, u, t0), (_, zp, Rp, _, t1) = sc["updates"][0], sc["updates"][1]
    zv, zp, u = zv[:B], np.nan_to_num(zp[:B], nan=0.1), u[:B]
    Rv, Rp = Rv[:B].copy(), Rp[:B].copy()
    Rv[1, 1, 0] = -1e-4     # zeroed
    Rv[2, 0, 0] = 0.0       # -> 1e-6
    Rv[3, 0, 0] = -2.0      # -> 0 -> 1e-6
    Rv[4, 0, 1] = -1e-4     # column 1 is never visited
    Rp[5, 1, 1] = -1e-5     # a negative R(1,1) is left alone (S stays positive: P(1,1) = 0.25)
    Rp[6, 2, 0] = -1e-5
    keep = (Rv.copy(), Rp.copy())
    ref.update_control(u)
    _cmp(worst, dev.update(0, zv, Rv, t0, u=u), ref.update(0, zv, Rv, t0))
    want = ref.update(1, zp, Rp, t1)
    _cmp(worst, dev.update(1, zp, Rp, t1), want)
    assert list(np.nonzero(want[3] & EC.R_REPAIRED)[0]) == [6]
    assert np.array_equal(Rv, keep[0]) and np.array_equal(Rp, keep[1])
    # the timestamp jumps back by 7.5 ms, then forward again: the negative dt integrates, nothing is reset
    for obs, z, R, t in ((0, zv, sc["updates"][0][2][:B], t1 - 7_500_000), (-1, None, None, t1 - 2_500_000), (1, zp, sc["updates"][1][2][:B], t1 + 5_000_000)):
        _cmp(worst, dev.update(obs, z, R, t), ref.update(obs, z, R, t))
        assert dev.get()["timestamp_ns"] == t
    print("check_cov and backward timestamp: |dx| %.2e |dP| %.2e |dKz| %.2e" % tuple(worst))
    assert max(worst) <= EC.TOL, worst


def test_euler_vehicle(pkg, sc):
    B = 64
    veh_d = dict(pkg.presets.barc_vehicle(), integrator="euler")
    veh = OP.barc_vehicle()
    veh.integrator = "euler"
    solver = pkg.Solver(pkg.presets.barc_tracking_mpc(20), veh_d, device=0)
    dev = _scenario_filter(solver, sc, B)
    ref = EC.new_filter(dict(sc, veh=veh), B=B)
    worst = [0.0, 0.0, 0.0]
    for obs, z, R, u, ns in sc["updates"][:20]:
        ref.update_control(u[:B])
        _cmp(worst, dev.update(obs, z, R, ns, u=u), ref.update(obs, z[:B], R[:B], ns))
    rk4 = EC.run(sc, B=B)[19]
    print("Euler, 20 updates: |dx| %.2e |dP| %.2e |dKz| %.2e (the RK4 filter is %.1e away)" % (*worst, np.abs(rk4[0] - ref.x).max()))
    assert max(worst) <= EC.TOL, worst
    assert np.abs(rk4[0] - ref.x).max() > 1e-7     # the integrator is really another one
    solver.close()


def test_misuse_is_an_argument_error_and_touches_nothing(solver, sc):
    import torch
    lib, h, B = solver.lib, solver._h, 8
    i32, i64 = C.c_int32, C.c_int64
    msg = lambda: lib.lmpc_last_error(h).decode()   # noqa: E731
    rows = lambda *r: (C.c_int32 * len(r))(*r)       # noqa: E731
    oid = C.c_int32(-7)
    dev = Dev(solver, sc["cfg"], B, (), sc["x0"], sc["P0"], initialize=False)
    kw = dict(dtype=torch.float64, device=solver.device)
    z, R, u = torch.zeros((2, B), **kw), torch.ones((2, 2, B), **kw), torch.zeros((2, B), **kw)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731

    def state():
        g = dev.get()
        return [g["x"].tobytes(), g["P"].tobytes(), g["K"].tobytes(), g["timestamp_ns"], g["initialized"]]

    before = state()
    assert lib.lmpc_ekf_initialize(h, i64(5)) == -1 and msg() == "No observation has been registered for the filter."
    for nz, r in ((0, rows(0)), (7, rows(0, 1, 2, 3, 4, 5, 0)), (2, rows(3, 3)), (2, rows(1, 6)), (1, rows(-1))):
        assert lib.lmpc_ekf_register_observation(h, i32(nz), r, C.byref(oid)) == -1 and "lmpc_ekf_register_observation" in msg(), (nz, list(r))
    assert oid.value == -7 and state() == before
    dev.ids = [solver.ekf_register_observation((3, 5))]
    before = state()
    args = (i32(0), p(z), p(R), i64(5_000_000), None, None, None, None)
    assert lib.lmpc_ekf_update_batch(h, i32(B), *args) == -1
    assert msg() == "Call EKFStateEstimator::initialize() before making any observation updates."
    assert state() == before
    solver.ekf_initialize(0)
    before = state()
    assert lib.lmpc_ekf_register_observation(h, i32(1), rows(4), C.byref(oid)) == -1
    assert msg() == "Changes to observations are not allowed after the filter is initialized."
    for bad_id in (1, -2):
        assert lib.lmpc_ekf_update_batch(h, i32(B), i32(bad_id), p(z), p(R), i64(5_000_000), None, None, None, None) == -1
        assert msg() == 'The observation name "%d" is not found.' % bad_id
    assert lib.lmpc_ekf_update_batch(h, i32(B), i32(0), None, p(R), i64(5_000_000), None, None, None, None) == -1
    for wrong in (B + 1, B - 1, 0):
        assert lib.lmpc_ekf_update_batch(h, i32(wrong), *args) == -1 and "batch" in msg()
        assert lib.lmpc_ekf_set_state(h, i32(wrong), None, None) == -1 and "batch" in msg()
        assert lib.lmpc_ekf_update_control(h, i32(wrong), p(u)) == -1 and "batch" in msg()
        assert lib.lmpc_ekf_get(h, i32(wrong), None, None, None, None, None) == -1 and "batch" in msg()
    assert lib.lmpc_ekf_update_control(h, i32(B), None) == -1
    assert state() == before
    assert lib.lmpc_ekf_update_batch(h, i32(B), *args) == 0          # and the filter still works
    solver.synchronize()
    assert dev.get()["timestamp_ns"] == 5_000_000
    solver.ekf_destroy()
    assert lib.lmpc_ekf_get(h, i32(B), None, None, None, None, None) == -1 and "lmpc_ekf_create" in msg()


def test_closed_loop_on_the_estimate(pkg, solver):
    """run_estimated on the BARC track: 64 cars, 200 periods of 25 ms, N = 20, start vx in [1.5, 2.5], the scenario's noise.  Everything
    is finite, every projection converges, no estimate goes non-finite; the recorded (u, z, t) of 8 cars replayed through the
    restatement gives the recorded estimates -- the filter is open-loop in them, so this holds whatever the controller does.
    RMS errors and failed solves are printed (profiles/ekf.md records them), not asserted."""
    import torch
    tr = pkg.racing_trajectory.RacingTrajectory(TC.BARC)
    spline = solver.spline_track(tr)
    tab = tr.to_track_table(1024)
    B, steps, nb = 64, 200, 8
    rng = np.random.default_rng(2)
    x0 = np.stack([rng.uniform(0, tab["L"], B), rng.uniform(-0.05, 0.05, B), np.zeros(B), rng.uniform(1.5, 2.5, B), np.zeros(B), np.zeros(B)])
    x0 = torch.as_tensor(x0, device=solver.device)
    u0 = torch.zeros((2, B), dtype=torch.float64, device=solver.device)
    res = pkg.closed_loop.run_estimated(solver, tab, spline, x0, u0, steps, seed=4, record_trace=True)
    plain = pkg.closed_loop.run_global(solver, tab, spline, x0, u0, steps)
    est_vx = np.array([t[5][3].cpu().numpy() for t in res["trace"]])
    print("run_estimated: rms error", res["rms_error"].cpu().numpy().round(4), "failed solves", int(res["n_fail"].sum()), "of", B * steps,
          "(run_global: %d)" % int(plain["n_fail"].sum()), "estimated vx %.2f .. %.2f" % (est_vx[20:].min(), est_vx.max()),
          "worst excess %.3f (run_global %.3f)" % (float(res["worst_excess"].max()), float(plain["worst_excess"].max())))
    for key in ("x", "x_est", "rms_error", "distance", "worst_excess"):
        assert bool(torch.isfinite(res[key]).all()), key
    assert (res["track_status"].cpu().numpy() == 0).all()
    assert not (res["ekf_flags"].cpu().numpy() & EC.NOT_FINITE).any()
    assert len(res["trace"]) == 2 * steps
    cfg = {k: np.asarray(v, dtype=np.float64) for k, v in res["ekf_config"].items()}
    ref = EC.Filter(OP.barc_vehicle(), cfg, nb)
    ref.register_observation(EC.ROWS_VEL)
    ref.register_observation(EC.ROWS_POSE)
    ref.set_state(Dev.host(res["x_est0"])[:nb], Dev.host(res["P0"])[:nb])
    ref.initialize(0)
    worst, n_drop = 0.0, 0
    for obs, z, R, u, ns, x_est in res["trace"]:
        ref.update_control(Dev.host(u)[:nb])
        x, _, _, fl = ref.update(obs, Dev.host(z)[:nb], Dev.host(R)[:nb], ns)
        worst = max(worst, float(np.abs(x - Dev.host(x_est)[:nb]).max()))
        n_drop += int((fl & EC.FALLBACK).sum())
    print("replay of %d cars: |dx| %.2e over %d updates, %d dropouts" % (nb, worst, len(res["trace"]), n_drop))
    assert n_drop > 0 and worst <= EC.TOL, worst


def test_cpp_class_driver(tmp_path):
    """EKFStateEstimator (host/ekf_state_estimator.hpp), one car, 50 updates against the restatement's numbers committed as
    tests/golden/ekf_one_car.npz; the driver raises each exception type once."""
    exe = LIB / "test_ekf"
    assert exe.exists(), "run __graft_entry__.build() first"
    g = np.load(ROOT / "tests" / "golden" / "ekf_one_car.npz")
    fmt = lambda a: " ".join(repr(float(v)) for v in np.asarray(a).reshape(-1))   # noqa: E731
    lines = [" ".join(fmt(g[k]) for k in ("x0", "P0", "Q", "x_min", "x_max"))]
    for i, o in enumerate(g["obs"]):
        nz = 0 if o < 0 else (2 if o == 0 else 3)
        lines.append(" ".join([str(int(o)), str(int(g["timestamp_ns"][i])), fmt(g["u"][i]), fmt(g["z"][i, :nz]), fmt(g["R"][i, :nz, :nz])]))
    run, out = tmp_path / "run.txt", tmp_path / "out.txt"
    run.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(run), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), (r.stdout[-2000:], r.stderr[-2000:])
    for sentence in ("No observation has been registered for the filter.", 'The observation name "pose" has already been registered.',
                     "Call EKFStateEstimator::initialize() before making any observation updates.",
                     "Changes to observations are not allowed after the filter is initialized.", 'The observation name "lidar" is not found.'):
        assert sentence in r.stdout, sentence
    got = np.loadtxt(out)
    assert got.shape == (50, 6 + 36 + 30 + 1)
    dx, dP = np.abs(got[:, :6] - g["x"]).max(), np.abs(got[:, 6:42] - g["P"].reshape(50, 36)).max()
    dK = np.abs(got[:, 42:72] - g["K"].reshape(50, 30)).max()
    print("C++ class, one car, 50 updates: |dx| %.2e |dP| %.2e |dK| %.2e" % (dx, dP, dK))
    assert max(dx, dP, dK) <= EC.TOL and np.array_equal(got[:, 72].astype(int), g["flags"])
