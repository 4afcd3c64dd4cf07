"""Shipped parameter sets of the reference, as plain dicts for the C ABI structs.

Transcribed from the reference's YAML (values only):
  vehicles  src/launch/racing_lmpc_launch/param/{barc,iac_car}/*_base.param.yaml, *_single_track.param.yaml
  MPC       src/launch/racing_lmpc_launch/param/racing_mpc/{barc_tracking_mpc,barc_lmpc,iac_car_tracking_mpc}.param.yaml
  vanilla   src/controllers/vanilla_controller/param/{vanilla_controller,vanilla_controller_2}.param.yaml
Field names are those of lmpc_vehicle / lmpc_config in include/lmpc_hip.h.
"""
from __future__ import annotations

INF = float("inf")


def barc_vehicle() -> dict:
    return dict(model_id=0, integrator="rk4", m=2.2187, Jzz=0.02723, l=0.324, cg_ratio=0.5, h=0.07, b=0.281, fr=0.012,
                kd=0.0, kb=0.5, cd=0.0, Af=1.0, rho=1.2, cl_f=0.0, cl_r=0.0, mu=0.9,
                Bf=5.0, Cf=2.28, Br=5.0, Cr=2.28, Fd_max=15.0, Fb_max=-15.0, Td=0.1, Tb=0.1,
                max_steer=0.314159, max_steer_rate=10.0)


def iac_vehicle() -> dict:
    return dict(model_id=0, integrator="rk4", m=811.9303, Jzz=700.0, l=2.9718, cg_ratio=0.45, h=0.35, b=2.0, fr=0.012,
                kd=0.0, kb=0.54, cd=1.0, Af=1.0, rho=1.2, cl_f=1.0, cl_r=1.0, mu=1.3,
                Bf=11.0, Cf=1.7, Br=11.0, Cr=1.7, Fd_max=10000.0, Fb_max=-20000.0, Td=0.1, Tb=0.1,
                max_steer=0.314159, max_steer_rate=0.66)


def barc_double_track() -> dict:
    """lmpc_vehicle_dt (include/lmpc_hip_dtrack.h) for the BARC car: barc_vehicle() with model_id 2 (LMPC_MODEL_DOUBLE_TRACK_PLANAR),
    chassis.tw_f / tw_r and front_tyre / rear_tyre pacejka_e / pacejka_fz0 / pacejka_eps of barc_base.param.yaml, kroll_f = 0.5 (the
    only value the reference ships, double_track_planar_model/param/sample_vehicle.param.yaml) and mu the single-track preset's."""
    return dict(barc_vehicle(), model_id=2, tw_f=0.281, tw_r=0.281, kroll_f=0.5,
                Ef=1.0, Fz0_f=1543.5, eps_f=-0.0813, Er=1.0, Fz0_r=1886.5, eps_r=-0.1263)


def iac_double_track() -> dict:
    """barc_double_track() for the IAC car, off iac_car_base.param.yaml."""
    return dict(iac_vehicle(), model_id=2, tw_f=1.6, tw_r=1.6, kroll_f=0.5,
                Ef=1.0, Fz0_f=1543.5, eps_f=-0.0813, Er=1.0, Fz0_r=1886.5, eps_r=-0.1263)


def barc_tracking_mpc(N: int = 20) -> dict:
    return dict(N=N, learning=0, num_ss_pts=96, num_ss_pts_per_lap=32, max_lap_stored=3, max_iter=0, tol=0.0,
                margin=0.1, q_contour=1.0, q_heading=1.0, q_vel=0.2, q_vy=1e-3, q_vyaw=1e-3, q_boundary=20.0,
                R=[0.01, 0.0, 0.0, 0.01], R_d=[0.01, 0.0, 0.0, 0.01],
                x_max=[INF, INF, INF, 6.0, 1.0, 3.0], x_min=[-INF, -INF, -INF, 0.1, -1.0, -3.0],
                u_max=[0.01, 0.33], u_min=[-0.01, -0.33],
                convex_hull_slack=[20.0, 20.0, 2.0, 20.0, 20.0, 2.0], max_vel_ref_diff=1.0)


def barc_lmpc(N: int = 20, n_laps: int = 3) -> dict:
    c = barc_tracking_mpc(N)
    c.update(learning=1, q_boundary=1000.0, R=[0.1, 0.0, 0.0, 0.1], R_d=[0.1, 0.0, 0.0, 0.1],
             x_max=[INF, INF, INF, 3.0, 1.0, 3.0], convex_hull_slack=[40.0, 40.0, 4.0, 40.0, 40.0, 4.0],
             num_ss_pts=32 * n_laps, num_ss_pts_per_lap=32, max_lap_stored=n_laps)
    return c


def iac_tracking_mpc(N: int = 40) -> dict:
    return dict(N=N, learning=0, num_ss_pts=96, num_ss_pts_per_lap=32, max_lap_stored=3, max_iter=0, tol=0.0,
                margin=0.5, q_contour=1.0, q_heading=1.0, q_vel=0.2, q_vy=0.01, q_vyaw=0.01, q_boundary=20.0,
                R=[1e-5, 0.0, 0.0, 1.0], R_d=[1e-4, 0.0, 0.0, 10.0],
                x_max=[INF, INF, INF, 100.0, 15.0, 2.0], x_min=[-INF, -INF, -INF, 3.0, -15.0, -2.0],
                u_max=[5.0, 0.314159], u_min=[-10.0, -0.314159],
                convex_hull_slack=[20.0, 20.0, 2.0, 20.0, 20.0, 2.0], max_vel_ref_diff=1.0)


def iac_lmpc(N: int = 60, n_laps: int = 3) -> dict:
    """iac_car_lmpc.param.yaml (n = 60): the IAC learning controller."""
    c = iac_tracking_mpc(N)
    c.update(learning=1, R=[1e-4, 0.0, 0.0, 1e-3], R_d=[5e-4, 0.0, 0.0, 1e-1],
             convex_hull_slack=[200.0, 20.0, 2.0, 200.0, 2.0, 20.0],
             num_ss_pts=32 * n_laps, num_ss_pts_per_lap=32, max_lap_stored=n_laps)
    return c


def sample_lqr(N: int = 20, dt: float = 0.01) -> dict:
    """Solver.lqr_create's config with the weights of mpc/racing_lqr/param/sample_lqr.param.yaml: Q = I, R = I (the two-control
    layout [u_lon, steer]; the file's 3 x 3 `r` is for a control layout this model does not have), Qf = diag(10, 10, 10, 1, 1, 10)."""
    eye = lambda d: [[float(d[i]) if i == j else 0.0 for j in range(len(d))] for i in range(len(d))]  # noqa: E731
    return dict(N=N, dt=dt, Q=eye([1.0] * 6), R=eye([1.0] * 2), Qf=eye([10.0, 10.0, 10.0, 1.0, 1.0, 10.0]))


def vanilla_controller(force_to_lon: float = 1e-3) -> dict:
    """Solver.vanilla_create's config with the values of controllers/vanilla_controller/param/vanilla_controller.param.yaml: a
    proportional speed controller (no integral, no derivative), lookahead one second of travel between 1 and 10 m.  force_to_lon is
    not in the file: 1e-3 hands the model the force the controller asked for, 1.0 is the reference's chain as written (newtons into a
    model whose unit is kN) -- include/lmpc_hip.h at lmpc_vanilla_create."""
    return dict(lookahead_speed_ratio=1.0, min_lookahead_distance=1.0, max_lookahead_distance=10.0,
                k_p=1.0, k_i=0.0, k_d=0.0, min_cmd=-5.0, max_cmd=5.0, min_i=0.0, max_i=0.0, dt=0.1, force_to_lon=force_to_lon)


def vanilla_controller_2(force_to_lon: float = 1e-3) -> dict:
    """vanilla_controller_2.param.yaml: lookahead between 3 and 40 m, a full PID (k_i = k_d = 0.1, integral within +- 3)."""
    return dict(lookahead_speed_ratio=1.0, min_lookahead_distance=3.0, max_lookahead_distance=40.0,
                k_p=1.0, k_i=0.1, k_d=0.1, min_cmd=-5.0, max_cmd=5.0, min_i=-3.0, max_i=3.0, dt=0.1, force_to_lon=force_to_lon)
