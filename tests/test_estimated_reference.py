"""The gate of the fused estimated period's tests, without a GPU: one period restated in numpy (tests/estimated_cases.py, from
ekf_cases.Filter, the host track class and the oracle's plant, shift and cold start) on the scenario the GPU tests run, and the
properties that scenario must have for those tests to mean something -- for every car the truth keeps vx >= 1.5 m/s (where the
filter does not depend on rounding), nothing is non-finite, every projection converges, and some but not all poses drop out.

No QP is solved here: the "solution" is the cold start's plan at x_ic with the drive of ekf_cases' scenario on it (the GPU tests take
a real solve), every seventh car declared failed."""
import numpy as np
import pytest

import ekf_cases as EC
import estimated_cases as XC
import track_cases as TC
from oracle import params as OP, scenario as S


@pytest.fixture(scope="module")
def track(pkg):
    tr = pkg.racing_trajectory.RacingTrajectory(TC.BARC)
    return tr, tr.to_track_table(1024)


def _one_period(track, N, B, restart):
    tr, tab = track
    cfg, veh = OP.barc_tracking_mpc(N), OP.barc_vehicle()
    sc = XC.scenario(float(tab["L"]), B)
    est0 = XC.global_state(tr, sc["x"]) + sc["est_noise"]
    frenet, res0 = XC.project(tr, est0[0:3], np.full(B, np.nan))
    x_ic = np.concatenate([frenet, est0[3:6]])
    inp = S.cold_start_inputs(cfg, veh, tab, x_ic.T, sc["u_prev"].T, XC.DT, speed_scale=XC.SPEED_SCALE)
    sol = {"X_optm": inp["X_ref"].copy(), "U_optm": inp["U_ref"].copy(), "status": sc["failed"].astype(np.int32)}
    sol["U_optm"][0] = 0.0018
    sol["U_optm"][1] = 0.05 * np.sin(np.arange(B))[None, :]
    filt = EC.Filter(veh, EC.config(), B)
    assert filt.register_observation(EC.ROWS_VEL) == 0 and filt.register_observation(EC.ROWS_POSE) == 1
    filt.set_state(est0.T, np.moveaxis(sc["P0"], -1, 0))
    filt.initialize(0)
    r = XC.period(tr, tab, cfg, veh, filt, inp, sol, sc["x"], x_ic, sc["noise_vel"], sc["R_vel"], sc["noise_pose"], sc["R_pose"], XC.DT_NS // 2,
                  XC.DT_NS, restart_failed=restart)
    return sc, inp, sol, x_ic, est0, res0, filt, r


@pytest.mark.parametrize("N,B", [(20, XC.WG + 1), (3, XC.WG + 1), (20, 1)])
def test_the_scenario_is_where_the_tests_mean_something(track, N, B):
    sc, inp, sol, x_ic, est0, res0, filt, r = _one_period(track, N, B, True)
    assert (sc["x"][3] >= 1.5).all() and (r["x"][3] >= 1.5).all(), float(r["x"][3].min())
    assert (est0[3] >= 1.3).all()
    for k in ("u", "x", "z_vel", "x_est", "sq_err", "x_ic", "distance", "excess") + XC.REF_KEYS:
        assert np.isfinite(r[k]).all(), k
    assert np.isfinite(r["z_pose"][1:]).all() and np.array_equal(np.isnan(r["z_pose"][0]), sc["dropped"])
    # every projection converges: the first-order condition (r(s) - p) . r'(s) = 0 holds at the abscissa returned, at the start and
    # behind the period.  The centre line is parametrised by arc length (|r'| = 1, H ~ 1), so the residual is the abscissa's error in
    # metres; the bound is ten times the 1e-9 the track tests hold the host class's abscissa to (track_cases.TOL_S) -- its line search
    # on the squared distance stalls there -- and six orders below a waypoint spacing.
    assert np.abs(res0).max() < 10 * TC.TOL_S and np.abs(r["residual"]).max() < 10 * TC.TOL_S
    assert not (r["flags"] & EC.NOT_FINITE).any()
    n_drop = int((r["flags"] & EC.FALLBACK != 0).sum())
    assert n_drop == int(sc["dropped"].sum())
    if B > 1:
        assert 0 < n_drop < B and 0 < int(sc["failed"].sum()) < B


@pytest.mark.parametrize("restart", [True, False])
def test_one_period_by_hand(track, restart):
    """What can be said about the period without running its parts again: who drove on which input, which cars took the pure
    prediction, what the next x_ic is made of, and where a failed car's next plan starts."""
    tr, tab = track
    B = XC.WG + 1
    sc, inp, sol, x_ic, est0, _, filt, r = _one_period(track, 20, B, restart)
    bad, ok = sc["failed"], ~sc["failed"]
    assert np.array_equal(r["u"][:, ok], sol["U_optm"][:, 0, ok]) and np.array_equal(r["u"][:, bad], inp["U_ref"][:, 0, bad])
    assert np.array_equal(r["fail"], bad.astype(np.int64)) and np.array_equal(filt.u, r["u"].T) and filt.ns == XC.DT_NS
    # the truth moved forward by about vx dt, and the filter knows nothing of it but through z
    assert np.allclose(r["distance"], sc["x"][3] * XC.DT, rtol=0.05)
    assert np.abs(r["z_vel"][0] - r["x"][3]).max() < 5 * EC.SIG_VEL[0] + 0.05   # (taken at mid-period: vx moves less than 0.05 in the other half)
    # a dropped pose: the car's estimate is the prediction from the velocity update, clipped
    twin = EC.Filter(OP.barc_vehicle(), EC.config(), B)
    twin.register_observation(EC.ROWS_VEL), twin.register_observation(EC.ROWS_POSE)
    twin.set_state(est0.T, np.moveaxis(sc["P0"], -1, 0))
    twin.initialize(0)
    twin.update_control(r["u"].T)
    twin.update(0, r["z_vel"].T, np.moveaxis(sc["R_vel"], -1, 0), XC.DT_NS // 2)
    xp, _, _, _ = twin.update(-1, None, None, XC.DT_NS)
    d = sc["dropped"]
    assert np.array_equal(xp[d].T, r["x_est"][:, d]) and not np.array_equal(xp[~d].T, r["x_est"][:, ~d])
    # the estimate is better than its start where the pose arrived (sd0 / 10 against the sensors' sigma)
    assert np.sqrt(r["sq_err"][0:2, ~d].mean()) < 0.03
    # x_ic: rows 3 - 5 the filter's, rows 0 - 2 the pose's projection -- taken back to the global frame it is the estimate's pose
    assert np.array_equal(r["x_ic"][3:6], r["x_est"][3:6])
    back = XC.global_state(tr, r["x_ic"])
    # (to the abscissa error the host class leaves, as above; the lateral offset and the heading follow the abscissa)
    assert np.abs(back[0:2] - r["x_est"][0:2]).max() < 10 * TC.TOL_S and np.abs(XC.wrap(back[2] - r["x_est"][2])).max() < 10 * TC.TOL_XI
    # the next plan: the solution moved one knot; a failed car's starts AT THE ESTIMATE (restart) or is the old plan moved one knot
    assert np.array_equal(r["X_ref"][:, :-1, ok], sol["X_optm"][:, 1:, ok])
    if restart:
        assert np.array_equal(r["X_ref"][:, 0, bad], r["x_ic"][:, bad]) and (r["U_ref"][:, :, bad] == 1e-9).all()
        assert np.abs(r["X_ref"][0:2, 0, bad] - r["x"][0:2, bad]).max() > 1e-6   # (not at the truth)
    else:
        assert np.array_equal(r["X_ref"][:, :-1, bad], inp["X_ref"][:, 1:, bad])
    assert np.array_equal(r["restarted"], bad if restart else np.zeros(B, dtype=bool))
