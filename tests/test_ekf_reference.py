"""The numpy restatement of the extended Kalman filter (tests/ekf_cases.py), checked on its own: against its extended-precision
twin on the scenario the device tests run, and property by property against ekf_state_estimator.cpp:112-264 as written."""
import numpy as np
import pytest

import ekf_cases as EC
from oracle import dynamics as D
from oracle import params as OP


@pytest.fixture(scope="module")
def sc():
    return EC.scenario(16)


def test_scenario_stays_in_the_well_conditioned_regime_and_the_twin_agrees(sc):
    """|fp64 - longdouble| <= 1e-13 in x and P after every one of the 800 updates: the reference's own rounding sensitivity, four
    orders below the device tolerance.  The true vx stays above 1.5 m/s, every estimate's vx (the seeds are floored at 0.5) inside RK4's
    stability bound 216 dt / vx < 2.78 at the 5 ms update, and yaw runs through +-pi."""
    a, b = EC.run(sc), EC.run(sc, np.longdouble)
    dx = max(np.abs(p[0] - q[0]).max() for p, q in zip(a, b))
    dP = max(np.abs(p[1] - q[1]).max() for p, q in zip(a, b))
    dK = max(np.abs(p[2] - q[2]).max() for p, q in zip(a, b))
    vx = np.array([p[0][:, 3] for p in a])
    vx_true = sc["truth"][:, :, 3]
    yaw = sc["truth"][:, :, 2]
    pmax = max(np.abs(p[1]).max() for p in a)
    print("twin: dx %.2e dP %.2e dK %.2e; est vx %.2f .. %.2f, true yaw %.2f .. %.2f, max |P| %.3f, true vx from %.2f" % (dx, dP, dK, vx.min(), vx.max(), yaw.min(), yaw.max(), pmax, vx_true.min()))
    assert all((p[3] == q[3]).all() for p, q in zip(a, b))
    assert dx <= EC.TOL_TWIN and dP <= EC.TOL_TWIN and dK <= EC.TOL_TWIN
    assert vx_true.min() >= 1.5 and 216 * 0.005 / min(vx.min(), sc["x0"][:, 3].min()) < 2.78 and yaw.max() > np.pi and yaw.min() < -np.pi and pmax <= 0.3
    drops = np.mean([(p[3] & EC.FALLBACK).mean() for p in a[1::2]])
    assert 0.05 < drops < 0.15 and not any((p[3] & EC.FALLBACK).any() for p in a[0::2])
    assert not any((p[3] & (EC.NOT_FINITE | EC.R_REPAIRED)).any() for p in a)


def _one(sc, B=4):
    f = EC.new_filter(sc, B=B)
    f.update_control(sc["updates"][0][3][:B])
    return f


def test_a_prediction_is_rk4_and_adds_q_once(sc):
    f = _one(sc)
    x0, P0, u = f.x.copy(), f.P.copy(), f.u.copy()
    x, P, Kz, fl = f.update(-1, None, None, 12_500_000)
    assert np.array_equal(x, np.clip(D.rk4(x0, u, 0.0, 0.0125, sc["veh"]), f.x_min, f.x_max)) and Kz is None and not fl.any()
    F = D.rk4_jacobian_cs(x0, u, 0.0, 0.0125, sc["veh"])[0]
    assert np.abs(P - (F @ P0 @ np.swapaxes(F, 1, 2) + np.diag(EC.Q_DIAG))).max() < 1e-13
    assert f.ns == 12_500_000 and (f.K == 0).all()


def test_a_nan_row_or_an_inf_in_r_gives_that_car_the_prediction(sc):
    obs, z, R, u, ns = sc["updates"][1]
    z, R = np.nan_to_num(z[:4], nan=0.3).copy(), R[:4].copy()
    ref, dirty, pred = _one(sc), _one(sc), _one(sc)
    xr, Pr, Kr, fr = ref.update(1, z, R, ns)
    z2, R2 = z.copy(), R.copy()
    z2[1, 2] = np.nan
    R2[3, 0, 1] = np.inf
    xd, Pd, Kd, fd = dirty.update(1, z2, R2, ns)
    xp, Pp, _, _ = pred.update(-1, None, None, ns)
    assert list(fd) == [0, EC.FALLBACK, 0, EC.FALLBACK] and not fr.any()
    for b in (1, 3):
        assert np.array_equal(xd[b], xp[b]) and np.array_equal(Pd[b], Pp[b]) and (Kd[b] == 0).all()
    for b in (0, 2):
        assert np.array_equal(xd[b], xr[b]) and np.array_equal(Pd[b], Pr[b]) and np.array_equal(Kd[b], Kr[b])


def test_the_clip_works_as_written(sc):
    cfg = EC.config(x_min=[-np.inf, -np.inf, -np.inf, 0.0, -0.01, -0.02], x_max=[np.inf, 0.1, np.inf, 1.0, 0.01, 0.02])
    f = EC.Filter(sc["veh"], cfg, 4)
    f.register_observation((3, 5))
    f.set_state(sc["x0"][:4], sc["P0"][:4])
    f.initialize(0)
    free = _one(sc)
    obs, z, R, u, ns = sc["updates"][0]
    f.update_control(u[:4])
    x, P, _, _ = f.update(0, z[:4], R[:4], ns)
    xf, Pf, _, _ = free.update(0, z[:4], R[:4], ns)
    assert np.array_equal(x, np.clip(xf, cfg["x_min"], cfg["x_max"])) and (x != xf).any()
    assert np.array_equal(P, Pf)   # P is untouched by the clip


def test_check_cov_visits_column_zero_only():
    R = np.array([[[0.0, 0.1], [-0.2, -0.3]], [[-1.0, -0.1], [0.2, 0.3]], [[0.5, -0.1], [0.2, 0.3]]])
    out, rep = EC.check_cov(R)
    assert np.array_equal(out[0], [[1e-6, 0.1], [0.0, -0.3]])    # R(0,0) = 0 -> 1e-6, R(1,0) < 0 -> 0, a negative R(1,1) is left alone
    assert np.array_equal(out[1], [[1e-6, -0.1], [0.2, 0.3]])    # R(0,0) < 0 -> 0 -> 1e-6, a negative R(0,1) is left alone
    assert np.array_equal(out[2], R[2]) and list(rep) == [True, True, False]
    assert R[0, 1, 0] == -0.2                                    # the caller's array is never written


def test_check_cov_reaches_the_update_and_is_flagged(sc):
    obs, z, R, u, ns = sc["updates"][0]
    R = R[:4].copy()
    R[1, 1, 0] = -1e-4
    R[2, 0, 0] = 0.0
    fixed = R.copy()
    fixed[1, 1, 0], fixed[2, 0, 0] = 0.0, 1e-6
    a, b = _one(sc), _one(sc)
    xa, Pa, Ka, fa = a.update(0, z[:4], R, ns)
    xb, Pb, Kb, fb = b.update(0, z[:4], fixed, ns)
    assert list(fa) == [0, EC.R_REPAIRED, EC.R_REPAIRED, 0] and not fb.any()
    assert np.array_equal(xa, xb) and np.array_equal(Pa, Pb) and np.array_equal(Ka, Kb)


def test_a_backward_timestamp_integrates_with_the_negative_dt(sc):
    f = _one(sc)
    f.update(-1, None, None, 20_000_000)
    x0, u = f.x.copy(), f.u.copy()
    x, P, _, _ = f.update(-1, None, None, 15_000_000)
    assert np.array_equal(x, D.rk4(x0, u, 0.0, -0.005, sc["veh"])) and f.ns == 15_000_000 and f.initialized


def test_an_update_overwrites_its_own_slice_of_the_gain_only(sc):
    f = _one(sc)
    (_, zv, Rv, _, t0), (_, zp, Rp, _, t1) = sc["updates"][0], sc["updates"][1]
    zp = np.nan_to_num(zp[:4], nan=0.1)
    f.update(1, zp, Rp[:4], t0)
    pose_slice = f.K[:, :, 2:5].copy()
    assert (f.K[:, :, 0:2] == 0).all() and (pose_slice != 0).any()
    _, _, Kz, _ = f.update(0, zv[:4], Rv[:4], t1)
    assert np.array_equal(f.K[:, :, 2:5], pose_slice) and np.array_equal(f.K[:, :, 0:2], Kz) and (Kz != 0).any()


def test_the_yaw_row_is_aligned_to_the_measurement(sc):
    """A pose measured one turn away gives the same innovation, so the same update: h is moved to the measurement's branch."""
    a, b = _one(sc), _one(sc)
    _, zp, Rp, _, ns = sc["updates"][1]
    zp = np.nan_to_num(zp[:4], nan=0.1)
    far = zp.copy()
    far[:, 2] += 2 * np.pi
    xa, Pa, _, _ = a.update(1, zp, Rp[:4], ns)
    xb, Pb, _, _ = b.update(1, far, Rp[:4], ns)
    assert np.abs(xa - xb).max() < 1e-12 and np.array_equal(Pa, Pb)
    naive = far[:, 2] - D.rk4(sc["x0"][:4], a.u, 0.0, ns * 1e-9, sc["veh"])[:, 2]
    assert (np.abs(naive) > 3.0).all()   # without the alignment the innovation would be a turn


def test_euler_vehicle_predicts_with_one_slope(sc):
    veh = OP.barc_vehicle()
    veh.integrator = "euler"
    f = EC.Filter(veh, sc["cfg"], 4)
    f.register_observation((3, 5))
    f.set_state(sc["x0"][:4], sc["P0"][:4])
    f.initialize(0)
    f.update_control(sc["updates"][0][3][:4])
    x0, P0 = f.x.copy(), f.P.copy()
    x, P, _, _ = f.update(-1, None, None, 5_000_000)
    fx, Fx, _ = D.f_and_partials(x0, f.u, 0.0, veh)
    assert np.abs(x - (x0 + 0.005 * fx)).max() < 1e-15
    F = D.rk4_jacobian_cs(x0, f.u, 0.0, 0.005, veh)[0]
    assert np.abs(P - (F @ P0 @ np.swapaxes(F, 1, 2) + np.diag(EC.Q_DIAG))).max() < 1e-13
