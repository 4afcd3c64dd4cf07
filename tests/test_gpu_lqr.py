"""The batched time-varying LQR on the device (lmpc_lqr_*) against the plain numpy restatement of tests/lqr_cases.py.

Tolerance lqr_cases.TOL = 1e-9 on X_optm, U_optm, K and P0, elementwise |d| / max(1, |reference|): 1e4 times the restatement's
measured distance from its extended-precision twin on the same scenarios at the same batch sizes (tests/test_lqr_reference.py), room
for FMA contraction, the device's atan / sin / tanh and another expm algorithm, each amplified by an N-step recursion; a wrong term
shows at 1e-3 or more.  Every scenario is one the CPU gate has qualified: every car checked there is checked here."""
import copy
import subprocess
from pathlib import Path

import numpy as np
import pytest

import lqr_cases as LC

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "racing-lmpc-ros2_amd" / "lib"
KEYS = ("X_optm", "U_optm", "K", "P0")

pytestmark = pytest.mark.gpu


def make_solver(pkg, kind="barc", **veh_over):
    veh = dict(pkg.presets.barc_vehicle() if kind == "barc" else pkg.presets.iac_vehicle(), **veh_over)
    return pkg.Solver(pkg.presets.barc_tracking_mpc(20), veh, device=0)


@pytest.fixture(scope="module")
def solvers(pkg):
    return {kind: make_solver(pkg, kind) for kind in ("barc", "iac")}


def dev(solver, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(np.moveaxis(np.asarray(a, dtype=np.float64), 0, -1)), device=solver.device)


def host(t):
    return np.moveaxis(t.cpu().numpy(), -1, 0)


def device_solve(solver, sc, max_batch=None, cars=None, **kw):
    """The scenario (its first `cars` cars) through the device: numpy arrays [B, ...] like the restatement's."""
    sl = slice(0, cars)
    B = sc["x_ic"][sl].shape[0]
    solver.lqr_create(sc["cfg"], B if max_batch is None else max_batch)
    out = solver.lqr_solve(dev(solver, sc["x_ic"][sl]), dev(solver, sc["X_ref"][sl]), dev(solver, sc["U_ref"][sl]), **kw)
    solver.synchronize()
    return {k: host(v) for k, v in out.items() if v is not None}


def check(got, ref, tol=LC.TOL, cars=None):
    worst = {k: LC.err(got[k], ref[k][:cars]) for k in KEYS}
    print({k: "%.1e" % v for k, v in worst.items()})
    for k in KEYS:
        assert got[k].shape == ref[k][:cars].shape, k
        assert worst[k] <= tol, (k, worst[k])
    assert np.array_equal(got["u"], got["U_optm"][:, :, 0])
    assert not got["flags"].any()


@pytest.mark.parametrize("key", LC.SCENARIOS, ids=lambda k: "-".join(str(v) for v in k))
def test_parity(solvers, key):
    """B = 67: eight full groups of a wave plus a partial wave and a partial group of 8; every car."""
    sc, ref = LC.reference(key)
    check(device_solve(solvers[sc["kind"]], sc, gains=True), ref)


def test_one_car(solvers):
    sc, ref = LC.reference(LC.SCENARIOS[2])
    check(device_solve(solvers["barc"], sc, cars=1, gains=True), ref, cars=1)


def test_batch_below_max_batch(solvers):
    """The workspace is laid out for the batch of the call: 67 cars on a store for 200 give the answer of a store for 67, bit for bit."""
    sc, ref = LC.reference(LC.SCENARIOS[3])
    got = device_solve(solvers["barc"], sc, max_batch=200, gains=True)
    check(got, ref)
    tight = device_solve(solvers["barc"], sc, gains=True)
    for k in KEYS:
        assert np.array_equal(got[k], tight[k]), k


def test_optional_outputs_and_repeatability(solvers):
    import torch
    sc, _ = LC.reference(LC.SCENARIOS[2])
    s = solvers["barc"]
    full = device_solve(s, sc, gains=True)
    again = device_solve(s, sc, gains=True)
    for k in KEYS + ("flags",):
        assert np.array_equal(full[k], again[k]), k
    B, N = sc["x_ic"].shape[0], sc["cfg"]["N"]
    kw = dict(dtype=torch.float64, device=s.device)
    bare = device_solve(s, sc, out={"X_optm": torch.empty((6, N, B), **kw), "U_optm": torch.empty((2, N - 1, B), **kw)})
    assert set(bare) == {"X_optm", "U_optm", "u"}
    assert np.array_equal(bare["X_optm"], full["X_optm"]) and np.array_equal(bare["U_optm"], full["U_optm"])
    plain = device_solve(s, sc)
    assert "K" not in plain and np.array_equal(plain["X_optm"], full["X_optm"]) and np.array_equal(plain["flags"], full["flags"])


def test_general_matrices(solvers):
    """Non-symmetric Q, Qf and a full non-symmetric R: P0 comes out non-symmetric, as the restatement's."""
    sc, ref = LC.reference(LC.GENERAL + ("general",))
    got = device_solve(solvers["barc"], sc, gains=True)
    check(got, ref)
    assert (np.abs(got["P0"] - np.swapaxes(got["P0"], 1, 2)).max(axis=(1, 2)) > 1e-3).all()


def test_euler_vehicle_gives_the_rk4_answer(pkg, solvers):
    """The class builds its own RK4 and does not read modeling.integrator_type."""
    sc, ref = LC.reference(LC.SCENARIOS[2])
    rk4 = device_solve(solvers["barc"], sc, gains=True)
    euler = device_solve(make_solver(pkg, "barc", integrator="euler"), sc, gains=True)
    for k in KEYS:
        assert np.array_equal(euler[k], rk4[k]), k
    check(euler, ref)
    veh = copy.copy(sc["veh"])
    veh.integrator = "euler"
    other = LC.euler_rollout(veh, sc["cfg"], sc["x_ic"], sc["X_ref"], sc["U_ref"], ref["K"])
    assert np.abs(euler["X_optm"] - other).max() > 1e-7


def test_one_cars_nan_stays_its_own(pkg, solvers):
    """A NaN reference, a reference at vx = 1e300 and a NaN start, planted in a batch of 67: those cars are flagged, the call
    succeeds, and every other car has the clean batch's bits.  (The kernels' loop counts are constants or N: nothing to lengthen.)"""
    sc, ref = LC.reference(LC.SCENARIOS[2])
    clean = device_solve(solvers["barc"], sc, gains=True)
    bad = dict(sc, x_ic=sc["x_ic"].copy(), X_ref=sc["X_ref"].copy())
    bad["X_ref"][5, 1, 7] = np.nan
    bad["X_ref"][40, 3, :] = 1e300
    bad["x_ic"][66, 2] = np.nan
    got = device_solve(solvers["barc"], bad, gains=True)
    planted = np.zeros(LC.B_TEST, dtype=bool)
    planted[[5, 40, 66]] = True
    assert (got["flags"][planted] == pkg.LQR_NOT_FINITE).all(), got["flags"][planted]
    assert not got["flags"][~planted].any()
    for k in KEYS:
        assert np.array_equal(got[k][~planted], clean[k][~planted]), k
    assert np.isnan(got["X_optm"][66]).any() and not np.isfinite(got["K"][5]).all() and not np.isfinite(got["K"][40]).all()
    assert np.isfinite(got["K"][66]).all()   # (its reference is clean: only the rollout carries the NaN)


def test_argument_errors(pkg, solvers):
    import torch
    s = solvers["barc"]
    sc, _ = LC.reference(LC.SCENARIOS[1])
    cfg = sc["cfg"]
    for wrong in (dict(cfg, N=1), dict(cfg, dt=0.0), dict(cfg, dt=-0.01), dict(cfg, dt=float("nan")), dict(cfg, dt=float("inf"))):
        with pytest.raises(pkg.LmpcError, match="-> -1"):
            s.lqr_create(wrong, 4)
    with pytest.raises(pkg.LmpcError, match="-> -1"):
        s.lqr_create(cfg, 0)
    s.lqr_create(cfg, 4)
    args = [dev(s, sc[k][:5]) for k in ("x_ic", "X_ref", "U_ref")]
    with pytest.raises(pkg.LmpcError, match="-> -1"):
        s.lqr_solve(*args)                        # batch 5 on a store for 4
    N = cfg["N"]
    X, U = torch.empty((6, N, 4), dtype=torch.float64, device=s.device), torch.empty((2, N - 1, 4), dtype=torch.float64, device=s.device)
    four = [dev(s, sc[k][:4]) for k in ("x_ic", "X_ref", "U_ref")]
    with pytest.raises(pkg.LmpcError, match="-> -1"):
        s.lqr_solve(*four, out={"X_optm": None, "U_optm": U})   # a null required pointer
    s.lqr_solve(*four, out={"X_optm": X, "U_optm": U})
    s.lqr_destroy()
    with pytest.raises(pkg.LmpcError, match="-> -1"):
        s.lqr_solve(*four)                        # after lmpc_lqr_destroy
    fresh = make_solver(pkg)
    with pytest.raises(pkg.LmpcError, match="-> -1"):
        fresh.lqr_solve(*[dev(fresh, sc[k][:4]) for k in ("x_ic", "X_ref", "U_ref")])   # before lmpc_lqr_create
    s.lqr_destroy()                               # nothing to destroy: LMPC_OK


def test_cpp_class_driver(solvers, tmp_path):
    """RacingLQR (host/racing_lqr.hpp), one car, on tests/golden/lqr_one_car.npz: the C ABI's bits at B = 1, the fixture's numbers."""
    exe = LIB / "test_racing_lqr"
    assert exe.exists(), "run __graft_entry__.build() first"
    g = np.load(ROOT / "tests" / "golden" / "lqr_one_car.npz")
    N = int(g["N"])
    fmt = lambda a: " ".join(repr(float(v)) for v in np.asarray(a).reshape(-1))   # noqa: E731
    case, out = tmp_path / "case.txt", tmp_path / "out.txt"
    case.write_text("\n".join(["%d %r" % (N, float(g["dt"]))] + [fmt(g[k]) for k in ("Q", "R", "Qf", "x_ic", "X_ref", "U_ref")]) + "\n")
    r = subprocess.run([str(exe), str(case), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), (r.stdout[-2000:], r.stderr[-2000:])
    lines = [np.array([float(v) for v in ln.split()]) for ln in out.read_text().splitlines()]
    assert len(lines) == 6
    got = {"X_optm": lines[0].reshape(1, 6, N), "U_optm": lines[1].reshape(1, 2, N - 1), "u": lines[2].reshape(1, 2),
           "K": lines[3].reshape(1, 2, 6, N - 1), "P0": lines[4].reshape(1, 6, 6), "flags": lines[5].astype(np.int32)}
    sc = {"cfg": LC.config(N, float(g["dt"]), g["Q"], g["R"], g["Qf"]), "x_ic": g["x_ic"][None], "X_ref": g["X_ref"][None], "U_ref": g["U_ref"][None]}
    abi = device_solve(solvers["barc"], sc, gains=True)
    for k in KEYS:
        assert np.array_equal(got[k], abi[k]), k
    check(got, {k: g[k][None] for k in KEYS})


def test_run_lqr(pkg, solvers):
    """closed_loop.run_lqr, 8 BARC cars, N = 21, 25 periods, against the same loop over the restatement, to 1e4 times the twin's
    distance on the loop itself (lqr_cases.TOL_LOOP)."""
    sc = LC.loop_scenario()
    s = solvers["barc"]
    s.lqr_create(sc["cfg"], LC.LOOP["B"])
    import torch
    res = pkg.closed_loop.run_lqr(s, dev(s, sc["x0"]), torch.as_tensor(sc["X_traj"], device=s.device), torch.as_tensor(sc["U_traj"], device=s.device),
                                  sc["steps"])
    s.synchronize()
    X, U = LC.run_loop(sc)
    ex, eu = LC.err(host(res["X"]), X), LC.err(host(res["U"]), U)
    print("run_lqr: X %.1e U %.1e" % (ex, eu))
    assert host(res["X"]).shape == X.shape and host(res["U"]).shape == U.shape
    assert not res["flags"].cpu().numpy().any()
    assert ex <= LC.TOL_LOOP and eu <= LC.TOL_LOOP, (ex, eu)
