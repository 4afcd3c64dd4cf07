"""One period of the estimated closed loop (lmpc_loop_advance_estimated_batch, include/lmpc_hip_estimated.h) restated in plain numpy
from the restatements the project already has -- the filter of tests/ekf_cases.py, the host track class the track tests hold the
device to (tests/track_cases.py), the oracle's plant, shift and cold start (oracle/scenario.py) -- and the scenario its tests run
(tests/test_estimated_reference.py without a GPU, tests/test_gpu_estimated_loop.py on one).

The scenario: the BARC track and vehicle, cars spread over the lap near the centre line at vx ~ U(1.5, 2.5) (the regime ekf_cases
pins: the model is stiff below), the filters started near the truth's pose, the sensors' noise of closed_loop.SENSORS with one pose
in ten dropped (a NaN in noise_pose[0]), every seventh solve declared failed.  Arrays carry the batch axis LAST, as the C ABI does."""
from __future__ import annotations

import numpy as np

import ekf_cases as EC
from oracle import scenario as S

REF_KEYS = ("X_ref", "U_ref", "T_ref", "bound_left", "bound_right", "curvatures", "vel_ref")
DT, N_SUB, SPEED_SCALE = 0.025, 2, 0.9
DT_NS = 25_000_000
WG = 64   # cars of a workgroup of lmpc_estimated_loop_kernel: the GPU tests run one full workgroup plus a lane, and a single car


def scenario(L: float, B: int, seed: int = 5, fail_every: int = 7) -> dict:
    """The draws of one period for B cars on a lap of length L: "x" [6][B] the truth (Frenet), "est_noise" [6][B] what is added to the
    truth's global state to start the filters (0.1 N(0, 1) sd0: vx stays above 1.3), "noise_vel" [2][B], "noise_pose" [3][B] (NaN in
    row 0 where the pose drops out), "R_vel" [2][2][B], "R_pose" [3][3][B], "P0" [6][6][B], "failed" [B] bool, "u_prev" [2][B]."""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(0, L, B), rng.uniform(-0.05, 0.05, B), rng.normal(0, 0.02, B), rng.uniform(1.5, 2.5, B), rng.normal(0, 0.02, B),
                  rng.normal(0, 0.1, B)])
    noise_pose = rng.normal(0, 1, (3, B)) * EC.SIG_POSE[:, None]
    drop = rng.random(B) < 0.1
    if B > 2:   # the property the tests need -- 0 < dropouts < B -- whatever the draw
        drop[1], drop[2] = True, False
    noise_pose[0, drop] = np.nan
    failed = np.zeros(B, dtype=bool)
    failed[::fail_every] = B > 1
    tile = lambda M: np.ascontiguousarray(np.moveaxis(np.tile(M, (B, 1, 1)), 0, -1))   # noqa: E731
    return {"x": x, "est_noise": 0.1 * rng.normal(0, 1, (6, B)) * EC.SD0[:, None], "noise_vel": rng.normal(0, 1, (2, B)) * EC.SIG_VEL[:, None],
            "noise_pose": noise_pose, "R_vel": tile(np.diag(EC.SIG_VEL ** 2)), "R_pose": tile(np.diag(EC.SIG_POSE ** 2)),
            "P0": tile(np.diag(EC.SD0 ** 2)), "failed": failed, "u_prev": rng.normal(0, 1e-3, (2, B)), "dropped": drop}


def wrap(a):
    return np.arctan2(np.sin(a), np.cos(a))


def global_state(tr, x):
    """[6][B] Frenet -> [6][B] global (pose, then the velocities as they are), by the host track class."""
    return np.stack(list(tr.frenet_to_global(x[0], x[1], x[2])) + [x[3], x[4], x[5]])


def project(tr, pose, s0):
    """RacingTrajectory.global_to_frenet per car, seeded with s0[b] where it is finite (else the nearest waypoint).
    -> (frenet [3][B], residual [B] of the first-order condition (r(s) - p) . r'(s) at the returned abscissa)."""
    B = pose.shape[1]
    out, res = np.empty((3, B)), np.empty(B)
    for b in range(B):
        out[:, b] = tr.global_to_frenet(pose[0, b], pose[1, b], pose[2, b], s0=float(s0[b]) if np.isfinite(s0[b]) else None)
        s = out[0, b]
        res[b] = (tr.x(s) - pose[0, b]) * tr._x(tr._mod(s), 1) + (tr.y(s) - pose[1, b]) * tr._y(tr._mod(s), 1)
    return out, res


def period(tr, tab, cfg, veh, filt, inp: dict, sol: dict, x, x_ic, noise_vel, R_vel, noise_pose, R_pose, t_vel_ns: int, t_pose_ns: int,
           dt: float = DT, n_sub: int = N_SUB, speed_scale: float = SPEED_SCALE, restart_failed: bool = True, obs=(0, 1)) -> dict:
    """Steps 1 - 8 of include/lmpc_hip_estimated.h.  tr: the host track class, tab: its uniform tables, cfg / veh: the oracle's
    config and vehicle, filt: an ekf_cases.Filter with the observations obs = (velocity, pose) registered; inp: REF_KEYS, sol:
    X_optm, U_optm, status; x [6][B] the truth, x_ic [6][B] what the solve was given.  The filter advances in place.
    -> "u", "x", "z_vel", "z_pose", "x_est" (global), "flags", "sq_err" [6][B], "x_ic", "residual" [B] (the projection's first-order
    condition), "distance", "excess", "fail", REF_KEYS (the next inputs), "restarted"."""
    L = float(tab["L"])
    ok = np.asarray(sol["status"]) == 0
    rows_v, rows_p = filt.obs[obs[0]][0], filt.obs[obs[1]][0]
    u = np.where(ok[None, :], sol["U_optm"][:, 0, :], inp["U_ref"][:, 0, :])                      # 1
    filt.update_control(u.T)
    x1 = S.plant_step(veh, tab, np.asarray(x).T, u.T, dt / n_sub, n_sub // 2)                     # 2
    z_vel = x1[:, rows_v] + noise_vel.T                                                           # 3
    _, _, _, f1 = filt.update(obs[0], z_vel, np.moveaxis(R_vel, -1, 0), t_vel_ns)
    x2 = S.plant_step(veh, tab, x1, u.T, dt / n_sub, n_sub // 2).T                                # 4
    ds = x2[0] - np.asarray(x)[0]
    half_b = float(veh.b) / 2.0
    truth = global_state(tr, x2)                                                                  # 5
    z_pose = truth[rows_p].T + noise_pose.T
    for a, r in enumerate(rows_p):
        if r == 2:
            z_pose[:, a] = wrap(z_pose[:, a])
    xe, _, _, f2 = filt.update(obs[1], z_pose, np.moveaxis(R_pose, -1, 0), t_pose_ns)
    xe = xe.T
    err = xe - truth                                                                              # 6
    err[2] = wrap(err[2])
    frenet, residual = project(tr, xe[0:3], np.asarray(x_ic)[0])                                  # 7
    x_ic_new = np.concatenate([frenet, xe[3:6]])
    plan_X = np.where(ok[None, None, :], sol["X_optm"], inp["X_ref"])                             # 8
    plan_U = np.where(ok[None, None, :], sol["U_optm"], inp["U_ref"])
    nxt = S.shift_inputs(cfg, veh, tab, plan_X, plan_U, dt, speed_scale=speed_scale)
    restarted = ~ok if restart_failed else np.zeros_like(ok)
    if restarted.any():
        cold = S.cold_start_inputs(cfg, veh, tab, x_ic_new.T, np.zeros((ok.size, 2)), dt, speed_scale=speed_scale)
        for k in REF_KEYS:
            nxt[k][..., restarted] = cold[k][..., restarted]
    out = {k: nxt[k] for k in REF_KEYS}
    out.update(u=u, x=x2, z_vel=z_vel.T, z_pose=z_pose.T, x_est=xe, flags=f1 | f2, sq_err=err ** 2, x_ic=x_ic_new, residual=residual,
               distance=np.where(ds < -L / 2.0, ds + L, ds), fail=(~ok).astype(np.int64), restarted=restarted,
               excess=np.maximum(x2[1] + half_b - inp["bound_left"][0], inp["bound_right"][0] - (x2[1] - half_b)))
    return out
