"""The numpy restatement of the batched vanilla controller (tests/vanilla_cases.py) -- no GPU.

The gate: every scenario the device tests run, on exactly their batches (B = 67, 1 / 2 / 64 periods, and the 700-period BARC run),
stays finite, keeps every car's body inside the track (worst_excess <= 0) and lies within TOL_TWIN / TOL_TWIN_ROLLOUT of its
extended-precision twin -- the measurement the device tolerances (1e4 times it) are derived from.  Then the restatement against
answers known in closed form, and the committed one-car fixture."""
from pathlib import Path

import numpy as np
import pytest

import track_cases as TC
import vanilla_cases as VC
from oracle import params as OP

ROOT = Path(__file__).resolve().parents[1]


# ---- the gate ----
@pytest.mark.parametrize("name", VC.SCENARIOS)
def test_gate_decision(name):
    worst = 0.0
    for what in ("decide", "decide_ref"):
        ref, twin = VC.reference(name, what), VC.reference(name, what, T=np.longdouble)
        assert not ref["flags"].any() and np.isfinite(ref["u_out"]).all() and np.isfinite(ref["u_model"]).all()
        worst = max(worst, VC.decision_err(ref, twin))
    print("%s: decision, restatement vs twin %.1e" % (name, worst))
    assert worst <= VC.TOL_TWIN, worst


@pytest.mark.parametrize("periods", (1, 2, VC.PERIODS))
@pytest.mark.parametrize("name", VC.SCENARIOS)
def test_gate_rollout(name, periods):
    ref, twin = VC.reference(name, "rollout", periods), VC.reference(name, "rollout", periods, T=np.longdouble)
    assert not ref["flags"].any()
    for k in VC.ROLLOUT_KEYS:
        assert np.isfinite(ref[k]).all(), k
    assert (ref["worst_excess"] <= 0.0).all(), ref["worst_excess"].max()
    d = VC.rollout_err(ref, twin)
    print("%s, %d periods: restatement vs twin %.1e, worst_excess %.3f" % (name, periods, d, ref["worst_excess"].max()))
    assert d <= VC.TOL_TWIN_ROLLOUT, d


def test_tolerances_follow_the_rule():
    assert VC.TOL == 1e4 * VC.TOL_TWIN and VC.TOL_ROLLOUT == 1e4 * VC.TOL_TWIN_ROLLOUT
    assert VC.TOL <= 1e-8 and VC.TOL_ROLLOUT <= 1e-8


def test_gate_long_run():
    """700 periods of the BARC scenario: finite, inside the track, and every car crosses the line twice -- one full lap closed."""
    sc = VC.scenario("barc")
    r = VC.rollout(sc["veh"], sc["cfg"], sc["trk"], sc["x0"], VC.zero_pid(VC.B_TEST), 700, sc["dt_sim"], sc["n_sub"], sc["speed_scale"])
    assert not r["flags"].any() and np.isfinite(r["X_log"]).all()
    assert (r["worst_excess"] <= 0.0).all(), r["worst_excess"].max()
    crossings = (np.diff(r["X_log"][:, 0], axis=1) < -sc["trk"]["L"] / 2).sum(axis=1)
    assert (crossings >= 2).all(), crossings.min()
    assert np.abs(r["U_log"][:, 1]).max() == sc["veh"].max_steer   # the steering clamp is exercised


def test_starts_are_the_issues():
    for name in VC.SCENARIOS:
        sc = VC.scenario(name)
        x0, L = sc["x0"], sc["trk"]["L"]
        assert x0.shape == (VC.B_TEST, 6) and (x0[:, 0] >= 0).all() and (x0[:, 0] < L).all()
        if sc["track"] == "barc":
            assert np.abs(x0[:, 1]).max() <= 0.1 and np.abs(x0[:, 2]).max() <= 0.1 and x0[:, 3].min() >= 1.0 and x0[:, 3].max() <= 2.0
    assert VC.scenario("preset2")["cfg"]["k_d"] == 0.1 and VC.scenario("force1")["cfg"]["force_to_lon"] == 1.0
    assert VC.scenario("barc")["cfg"]["force_to_lon"] == 1e-3 and VC.scenario("barc")["speed_scale"] == 0.5


# ---- known answers ----
def circle_track(R: float = 50.0, n: int = 1600) -> dict:
    th = np.arange(n) * 2 * np.pi / n
    tab = np.zeros((n, 17))
    tab[:, 0], tab[:, 1] = R * np.cos(th), R * np.sin(th)
    tab[:, 4] = 20.0
    tab[:, 6], tab[:, 7] = R * th, 2 * np.pi * R
    tab[:, 9], tab[:, 10] = (R - 5.0) * np.cos(th), (R - 5.0) * np.sin(th)     # left of a counter-clockwise curve: inside
    tab[:, 11], tab[:, 12] = (R + 5.0) * np.cos(th), (R + 5.0) * np.sin(th)
    tr = VC.pkg().racing_trajectory.RacingTrajectory(tab)
    return {"spline": tr.to_spline_track(), "table": tr.to_track_table(VC.TABLE_M), "L": tr.total_length, "tr": tr}


def test_centre_line_at_the_reference_speed():
    """On a circle of radius R, on the centre line, heading along it: the chord to the point an arc la ahead makes the angle
    la / (2 R) with the tangent, so STEER = atan(2 l sin(la / 2R) / la); at v = vel_ref the PID asks for nothing and F = roll + aero."""
    R, veh = 50.0, OP.iac_vehicle()
    trk = circle_track(R)
    cfg = VC.barc_config(lookahead_speed_ratio=0.5, min_lookahead_distance=5.0, max_lookahead_distance=40.0)
    s = np.array([3.0, 100.0, 250.0, 313.0])
    v = np.array([8.0, 20.0, 30.0, 100.0])            # la = 5 (the minimum), 10, 15, 40 (the maximum)
    x = np.stack([s, 0 * s, 0 * s, v, 0 * s, 0 * s], axis=1)
    r = VC.decide(veh, cfg, trk, x, VC.zero_pid(4), vel_ref=v)
    la = np.array([5.0, 10.0, 15.0, 40.0])
    np.testing.assert_allclose(r["la"], la, rtol=0, atol=0)
    np.testing.assert_allclose(np.sin(r["alpha"]), np.sin(la / (2 * R)), rtol=0, atol=1e-8)   # (a cubic through waypoints h = 0.2 m apart: tangent error h^3 / (24 R^3) = 3e-9)
    np.testing.assert_allclose(r["u_out"][:, 2], np.arctan(2 * veh.l * np.sin(la / (2 * R)) / la), rtol=0, atol=1e-8)
    aero = 0.5 * veh.rho * veh.Af * veh.cd * v * v
    F = veh.fr * (veh.m * 9.81 + aero * (veh.cl_f + veh.cl_r)) + aero
    np.testing.assert_allclose(r["u_out"][:, 0], F, rtol=1e-15)
    assert (r["u_out"][:, 1] == 0).all() and (r["cmd"] == 0).all()
    # vel_ref NULL: the spline's 20 m/s times speed_scale
    r2 = VC.decide(veh, cfg, trk, x[1:2], VC.zero_pid(1), None, speed_scale=1.0)
    assert abs(r2["pid"]["error"][0]) < 1e-12
    r3 = VC.decide(veh, cfg, trk, x[1:2], VC.zero_pid(1), None, speed_scale=0.5)
    np.testing.assert_allclose(r3["pid"]["error"], [-10.0], atol=1e-12)


def pid_cfg(**over):
    return VC.barc_config(**dict(dict(k_p=2.0, k_i=0.5, k_d=0.1, min_cmd=-5.0, max_cmd=5.0, min_i=-0.3, max_i=0.2, dt=0.1), **over))


def test_pid_known_answers():
    T = np.float64
    one = lambda v: np.array([v], dtype=T)   # noqa: E731
    cfg = pid_cfg()
    # the first call's derivative sees e / dt, as upstream (last_error starts at 0)
    cmd, st = VC.pid_update(cfg, VC.zero_pid(1), one(1.0), T)
    assert st["error"][0] == 1.0 and st["last_error"][0] == 0.0 and st["integral"][0] == 0.1
    assert cmd[0] == 2.0 * 1.0 + 0.1 * 0.5 + (1.0 - 0.0) / 0.1 * 0.1
    # second call: the integral clamps at max_i, the derivative is the difference
    cmd, st2 = VC.pid_update(cfg, st, one(1.5), T)
    assert st2["integral"][0] == 0.2 and st2["last_error"][0] == 1.0 and st2["error"][0] == 1.5
    assert cmd[0] == 1.5 * 2.0 + 0.2 * 0.5 + (1.5 - 1.0) / 0.1 * 0.1
    # ... and at min_i
    _, st3 = VC.pid_update(cfg, st2, one(-9.0), T)
    assert st3["integral"][0] == -0.3
    # the output clamps are <= and >=: a command exactly on a limit is the limit, beyond it too
    flat = pid_cfg(k_p=1.0, k_i=0.0, k_d=0.0)
    for e, want in ((5.0, 5.0), (7.0, 5.0), (-5.0, -5.0), (-7.0, -5.0), (4.999, 4.999)):
        assert VC.pid_update(flat, VC.zero_pid(1), one(e), T)[0][0] == want
    # NaN in: NaN out, state unchanged
    cmd, st4 = VC.pid_update(cfg, st2, one(np.nan), T)
    assert np.isnan(cmd[0]) and all(st4[k][0] == st2[k][0] for k in VC.PID_KEYS)


def test_split_fold_force_to_lon_and_flag():
    sc = VC.scenario("barc")
    veh, trk = sc["veh"], sc["trk"]
    x = sc["x0"][:4].copy()
    v = np.hypot(x[:, 3], x[:, 4])
    cfg = VC.barc_config(k_i=0.0)
    roll = veh.fr * veh.m * 9.81
    up = VC.decide(veh, cfg, trk, x, VC.zero_pid(4), vel_ref=v + 1.0)       # cmd = +1: F = m + roll > 0 -> (F, 0)
    dn = VC.decide(veh, cfg, trk, x, VC.zero_pid(4), vel_ref=v - 1.0)       # cmd = -1: F = -m + roll < 0 -> (0, F)
    np.testing.assert_allclose(up["u_out"][:, 0], veh.m * 1.0 + roll, rtol=1e-12)
    assert (up["u_out"][:, 1] == 0).all()
    np.testing.assert_allclose(dn["u_out"][:, 1], -veh.m * 1.0 + roll, rtol=1e-12)
    assert (dn["u_out"][:, 0] == 0).all()
    # the fold picks the non-zero one; u_model = (u_a force_to_lon, STEER)
    assert np.array_equal(up["u_model"][:, 0], up["u_out"][:, 0] * 1e-3) and np.array_equal(dn["u_model"][:, 0], dn["u_out"][:, 1] * 1e-3)
    assert np.array_equal(up["u_model"][:, 1], up["u_out"][:, 2])
    one = VC.decide(veh, dict(cfg, force_to_lon=1.0), trk, x, VC.zero_pid(4), vel_ref=v + 1.0)
    assert np.array_equal(one["u_model"][:, 0], one["u_out"][:, 0]) and np.array_equal(one["u_out"], up["u_out"])
    # F = 0 exactly goes to FB (`ctrl_force > 0.0` is false), and the fold then returns FB = 0
    nofr = OP.barc_vehicle()
    nofr.fr = 0.0
    z = VC.decide(nofr, cfg, trk, x, VC.zero_pid(4), vel_ref=v)
    assert (z["u_out"][:, :2] == 0).all() and (z["u_model"][:, 0] == 0).all()
    # the flag: a NaN state, an abscissa beyond LAPS_MAX laps, a NaN vel_ref -- flagged, PID state untouched, the others' bits unchanged
    bad, vr = x.copy(), v + 1.0
    bad[0, 1], bad[1, 0], vr[2] = np.nan, 1e300, np.nan
    pid = {k: np.full(4, 0.25) for k in VC.PID_KEYS}
    b = VC.decide(veh, cfg, trk, bad, pid, vel_ref=vr)
    assert list(b["flags"]) == [1, 1, 1, 0]
    assert all((b["pid"][k][:3] == 0.25).all() for k in VC.PID_KEYS)
    clean = VC.decide(veh, cfg, trk, x, pid, vel_ref=v + 1.0)
    assert np.array_equal(b["u_out"][3], clean["u_out"][3]) and not np.isfinite(b["u_out"][:3]).all(axis=1).any()


def test_rollout_freezes_a_car_that_turns_non_finite():
    sc = VC.scenario("barc")
    x0 = sc["x0"][:5].copy()
    x0[1, 5] = np.nan            # omega: the decision does not read it, the plant does
    x0[3, 0] = 1e300
    r = VC.rollout(sc["veh"], sc["cfg"], sc["trk"], x0, VC.zero_pid(5), 4, sc["dt_sim"], sc["n_sub"], sc["speed_scale"])
    clean = VC.rollout(sc["veh"], sc["cfg"], sc["trk"], sc["x0"][:5], VC.zero_pid(5), 4, sc["dt_sim"], sc["n_sub"], sc["speed_scale"])
    assert list(r["flags"]) == [0, 1, 0, 1, 0]
    for b in (1, 3):
        assert np.isnan(r["X_log"][b]).all() and np.isnan(r["U_log"][b]).all() and np.isnan(r["k_log"][b]).all()
        assert np.array_equal(r["x"][b], x0[b], equal_nan=True) and r["distance"][b] == 0 and r["worst_excess"][b] == -np.inf
        assert all(r["pid"][k][b] == 0 for k in VC.PID_KEYS)
    for b in (0, 2, 4):
        for k in VC.ROLLOUT_KEYS:
            assert np.array_equal(r[k][b], clean[k][b]), k


def test_chunks_compose():
    """Two rollouts of 32 periods, the second from where the first ended, are one of 64."""
    sc = VC.scenario("barc")
    whole = VC.reference("barc", "rollout", 64)
    a = VC.rollout(sc["veh"], sc["cfg"], sc["trk"], sc["x0"], VC.zero_pid(VC.B_TEST), 32, sc["dt_sim"], sc["n_sub"], sc["speed_scale"])
    b = VC.rollout(sc["veh"], sc["cfg"], sc["trk"], a["x"], a["pid"], 32, sc["dt_sim"], sc["n_sub"], sc["speed_scale"],
                   distance=a["distance"], worst_excess=a["worst_excess"])
    assert np.array_equal(b["x"], whole["x"]) and np.array_equal(np.concatenate([a["X_log"], b["X_log"]], axis=2), whole["X_log"])
    assert np.array_equal(b["worst_excess"], whole["worst_excess"]) and np.array_equal(b["distance"], whole["distance"])
    assert all(np.array_equal(b["pid"][k], whole["pid"][k]) for k in VC.PID_KEYS)


def test_committed_one_car_fixture(golden):
    g = golden("vanilla_one_car")
    sc = VC.scenario("barc", B=1)
    cfg = dict(zip((str(n) for n in g["cfg_names"]), (float(v) for v in g["cfg_values"])))
    assert cfg == sc["cfg"] and np.array_equal(g["x0"], sc["x0"][0])
    P = g["k_log"].shape[0]
    assert P == 64 and g["X_log"].shape == (6, 64) and g["U_log"].shape == (2, 64) and g["u_out"].shape == (64, 3)
    r = VC.rollout(sc["veh"], cfg, sc["trk"], g["x0"][None], VC.zero_pid(1), P, float(g["dt_sim"]), int(g["n_sub"]), float(g["speed_scale"]))
    for k in VC.ROLLOUT_KEYS:
        assert VC.err(r[k][0], g[k]) <= 1e-12, k     # (numpy's transcendental functions may differ by an ulp between builds)
    assert VC.err(np.array([r["pid"][k][0] for k in VC.PID_KEYS]), g["pid"]) <= 1e-12
    # the fold of the logged decisions is the logged command
    ua = np.where(np.abs(g["u_out"][:, 0]) > np.abs(g["u_out"][:, 1]), g["u_out"][:, 0], g["u_out"][:, 1])
    assert np.array_equal(ua * cfg["force_to_lon"], g["U_log"][0]) and np.array_equal(g["u_out"][:, 2], g["U_log"][1])


def test_presets_match_the_parameter_files():
    pkg = VC.pkg()
    d = ROOT / "tests" / "golden" / "ros_params" / "vanilla_controller"
    for name in ("vanilla_controller", "vanilla_controller_2"):
        got = pkg.ros_params.vanilla_config_from_params(pkg.ros_params.load_ros_params(d / f"{name}.param.yaml"))
        assert got.pop("step_mode") == "continuous"
        assert got == getattr(pkg.presets, name)()
        assert pkg.ros_params.vanilla_config_from_params(pkg.ros_params.load_ros_params(d / f"{name}.param.yaml"), 1.0)["force_to_lon"] == 1.0
    params = pkg.ros_params.load_ros_params(d / "vanilla_controller.param.yaml")
    with pytest.raises(KeyError, match="lon_kp"):
        pkg.ros_params.vanilla_config_from_params({k: v for k, v in params.items() if not k.endswith("lon_kp")})
    with pytest.raises(ValueError, match="Invalid step mode"):
        pkg.ros_params.vanilla_config_from_params(dict(params, **{"vanilla_controller.step_mode": "other"}))
    assert TC.BARC.exists()
