"""The LQR's numpy restatement (tests/lqr_cases.py) held to its extended-precision twin and to known answers, on the CPU.

The first test is the gate that keeps a device test from hiding behind a bad scenario: on every scenario the device tests use, at
their batch sizes, the float64 restatement and the longdouble twin agree to TOL_TWIN, every car stays within 2 m (BARC) or 20 m
(IAC) of its reference, and nothing is non-finite.  No car is left out."""
from pathlib import Path

import numpy as np
import pytest

import lqr_cases as LC
from oracle import dynamics as D

ROOT = Path(__file__).resolve().parents[1]
KEYS = ("X_optm", "U_optm", "K", "P0")


@pytest.mark.parametrize("key", list(LC.SCENARIOS) + [LC.GENERAL + ("general",)], ids=lambda k: "-".join(str(v) for v in k))
def test_scenarios_qualify(key):
    sc, ref = LC.reference(key)
    assert sc["x_ic"].shape[0] == LC.B_TEST
    twin = LC.solve(sc["veh"], sc["cfg"], sc["x_ic"], sc["X_ref"], sc["U_ref"], np.longdouble)
    e = {k: LC.err(ref[k], twin[k]) for k in KEYS}
    dev = np.abs(ref["X_optm"] - sc["X_ref"]).max(axis=(1, 2))
    print(key, {k: "%.1e" % v for k, v in e.items()}, "max |X_optm - X_ref| %.3f" % dev.max())
    assert not ref["flags"].any() and not twin["flags"].any()
    for k in KEYS:
        assert np.isfinite(ref[k]).all(), k
        assert e[k] <= LC.TOL_TWIN, (k, e[k])
    assert (dev < LC.MAX_DEVIATION[sc["kind"]]).all(), dev.max()


def test_loop_scenario_qualifies():
    sc = LC.loop_scenario()
    X, U = LC.run_loop(sc)
    Xt, Ut = LC.run_loop(sc, np.longdouble)
    ex, eu = LC.err(X, Xt), LC.err(U, Ut)
    print("loop: X %.1e U %.1e" % (ex, eu))
    assert np.isfinite(X).all() and np.isfinite(U).all()
    assert ex <= LC.TOL_TWIN_LOOP and eu <= LC.TOL_TWIN_LOOP, (ex, eu)
    assert np.abs(X - sc["X_traj"][:, :, :X.shape[2]]).max() < LC.MAX_DEVIATION["barc"]


def test_tolerances_follow_the_rule():
    assert LC.TOL == 1e4 * LC.TOL_TWIN and LC.TOL <= 1e-8
    assert LC.TOL_LOOP == 1e4 * LC.TOL_TWIN_LOOP and LC.TOL_LOOP <= 1e-8


def test_on_the_reference_the_plan_is_the_reference():
    sc, _ = LC.reference(LC.SCENARIOS[2])
    r = LC.solve(sc["veh"], sc["cfg"], sc["X_ref"][:, :, 0], sc["X_ref"], sc["U_ref"])
    assert np.array_equal(r["U_optm"], sc["U_ref"])
    assert np.abs(r["X_optm"] - sc["X_ref"]).max() <= 1e-13


def test_one_stage_gain_directly():
    """N = 2: K_0 = (R + B'Qf B)^-1 B'Qf A with A, B from the series of the matrix exponential."""
    sc, ref = LC.reference(LC.SCENARIOS[0])
    cfg, veh = sc["cfg"], sc["veh"]
    _, Ac, Bc = D.f_and_partials(sc["X_ref"][:, :, 0], sc["U_ref"][:, :, 0], 0.0, veh)
    A, Bd = series(Ac, Bc, cfg["dt"])
    Bt = np.swapaxes(Bd, 1, 2)
    K0 = np.linalg.inv(cfg["R"] + Bt @ cfg["Qf"] @ Bd) @ Bt @ cfg["Qf"] @ A
    assert LC.err(ref["K"][:, :, :, 0], K0) <= 1e-12
    P0 = cfg["Q"] + np.swapaxes(A, 1, 2) @ cfg["Qf"] @ (A - Bd @ K0)
    assert LC.err(ref["P0"], P0) <= 1e-12


def series(Ac, Bc, dt, terms: int = 60):
    """A = sum (Ac dt)^j / j!,  B = sum (Ac dt)^j / (j+1)! Bc dt."""
    nb = Ac.shape[0]
    term = np.broadcast_to(np.eye(6), (nb, 6, 6)).copy()
    A, S = term.copy(), term.copy()
    for j in range(1, terms):
        term = term @ (Ac * dt) / j
        A = A + term
        S = S + term / (j + 1)
    return A, S @ Bc * dt


def test_expm_block_against_the_series():
    for key in (LC.SCENARIOS[2], LC.SCENARIOS[5]):   # BARC and IAC
        sc, ref = LC.reference(key)
        k = 3
        _, Ac, Bc = D.f_and_partials(sc["X_ref"][:, :, k], sc["U_ref"][:, :, k], 0.0, sc["veh"])
        A, Bd = series(Ac, Bc, sc["cfg"]["dt"])
        assert LC.err(ref["A"][:, k], A) <= 1e-12 and LC.err(ref["B"][:, k], Bd) <= 1e-12
        A2, B2 = LC.discretize(Ac, Bc, sc["cfg"]["dt"], np.longdouble)
        assert LC.err(A2, A) <= 1e-12 and LC.err(B2, Bd) <= 1e-12
        assert np.abs(A - np.eye(6)).max() > 1e-3   # (not the identity: a missing dt would show)


def test_general_matrices_are_not_symmetrised():
    sc, ref = LC.reference(LC.GENERAL + ("general",))
    cfg = sc["cfg"]
    assert np.abs(cfg["Q"] - cfg["Q"].T).max() > 0.01 and np.abs(cfg["R"] - cfg["R"].T).max() > 0.01
    asym = np.abs(ref["P0"] - np.swapaxes(ref["P0"], 1, 2)).max(axis=(1, 2))
    assert (asym > 1e-3).all(), asym.min()
    # the symmetrised weights give another answer: the restatement uses what it is given
    sym = dict(cfg, Q=(cfg["Q"] + cfg["Q"].T) / 2, R=(cfg["R"] + cfg["R"].T) / 2, Qf=(cfg["Qf"] + cfg["Qf"].T) / 2)
    other = LC.solve(sc["veh"], sym, sc["x_ic"], sc["X_ref"], sc["U_ref"])
    assert LC.err(other["K"], ref["K"]) > 1e-4


def test_euler_vehicle_takes_the_rk4_rollout():
    import copy
    sc, ref = LC.reference(LC.SCENARIOS[2])
    veh = copy.copy(sc["veh"])
    veh.integrator = "euler"
    r = LC.solve(veh, sc["cfg"], sc["x_ic"], sc["X_ref"], sc["U_ref"])
    assert np.array_equal(r["X_optm"], ref["X_optm"])
    assert np.abs(LC.euler_rollout(veh, sc["cfg"], sc["x_ic"], sc["X_ref"], sc["U_ref"], ref["K"]) - ref["X_optm"]).max() > 1e-7


def test_one_car_fixture_is_reproduced():
    g = np.load(ROOT / "tests" / "golden" / "lqr_one_car.npz")
    cfg = LC.config(int(g["N"]), float(g["dt"]), g["Q"], g["R"], g["Qf"])
    r = LC.solve(LC.vehicle("barc"), cfg, g["x_ic"][None], g["X_ref"][None], g["U_ref"][None])
    for k in KEYS:
        assert LC.err(r[k][0], g[k]) <= LC.TOL_TWIN, k
