"""ctypes binding of include/lmpc_hip.h (lib/liblmpc_hip.so).

`Solver` mirrors the reference's RacingMPC surface for a whole batch: it is constructed from a
config and a vehicle (RacingMPC::RacingMPC, racing_mpc.cpp:31-35) and `solve()` takes/returns the
same keys as RacingMPC::solve's DMDict (racing_mpc.cpp:215-228, 347-353) with a trailing batch
axis.  Tensors are torch CUDA (ROCm) fp64 tensors; only their device pointers cross the ABI.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

_HERE = Path(__file__).resolve().parent
_LIB = None

SOLVE_OPTIMAL, SOLVE_MAX_ITER, SOLVE_INFEASIBLE = 0, 1, 2
TRACK_OK, TRACK_NOT_CONVERGED, TRACK_BAD_INPUT = 0, 1, 2   # per-pose status of Solver.global_to_frenet

_ABI_SYMBOLS = ("lmpc_create", "lmpc_destroy", "lmpc_last_error", "lmpc_set_stream", "lmpc_synchronize",
                "lmpc_linearize_batch", "lmpc_solve_batch", "lmpc_set_safe_set", "lmpc_ss_query_batch",
                "lmpc_prepare_batch", "lmpc_reserve", "lmpc_query_launch", "lmpc_enable_timing",
                "lmpc_last_kernel_ms", "lmpc_query_residency", "lmpc_query_launch_for", "lmpc_solve_host", "lmpc_shift_batch",
                "lmpc_plant_step_batch", "lmpc_solve_full_dynamics_batch", "lmpc_solve_full_dynamics_host", "lmpc_set_regression_laps", "lmpc_regress_batch", "lmpc_ss_query_host", "lmpc_solve_batch_f32",
                "lmpc_solve_batch_mixed", "lmpc_prepare_failed_batch", "lmpc_set_launch_order", "lmpc_set_warm_rounds", "lmpc_loop_advance_batch", "lmpc_launch_order_from_iters", "lmpc_set_output_layout",
                "lmpc_ss_query_idx_batch", "lmpc_solve_batch_ss_idx", "lmpc_solve_batch_warm", "lmpc_solve_host_warm",
                "lmpc_last_solve_precision", "lmpc_solve_batch_warm_ss", "lmpc_solve_host_warm_ss", "lmpc_shift_lambda_batch",
                "lmpc_get_warm_accepted", "lmpc_set_waves_per_problem",
                "lmpc_fleet_ss_create", "lmpc_fleet_ss_destroy", "lmpc_fleet_ss_reset", "lmpc_fleet_ss_bytes", "lmpc_fleet_ss_record_batch",
                "lmpc_fleet_ss_query_batch", "lmpc_fleet_ss_load", "lmpc_fleet_ss_get_laps", "lmpc_fleet_ss_stats",
                "lmpc_fleet_ss_set_regression", "lmpc_fleet_ss_regress_batch", "lmpc_fleet_loop_advance_batch",
                "lmpc_spline_track_create", "lmpc_spline_track_destroy", "lmpc_spline_track_tabulate", "lmpc_track_sample_batch",
                "lmpc_global_to_frenet_batch", "lmpc_frenet_to_global_batch",
                "lmpc_ekf_create", "lmpc_ekf_destroy", "lmpc_ekf_register_observation", "lmpc_ekf_initialize", "lmpc_ekf_set_state",
                "lmpc_ekf_update_control", "lmpc_ekf_update_batch", "lmpc_ekf_get",
                "lmpc_lqr_create", "lmpc_lqr_destroy", "lmpc_lqr_solve_batch",
                "lmpc_vanilla_create", "lmpc_vanilla_destroy", "lmpc_vanilla_reset", "lmpc_vanilla_get", "lmpc_vanilla_solve_batch",
                "lmpc_vanilla_rollout_batch")
# the entry points of include/lmpc_hip_rows.h (one feature list per regressed row), resolved at load time with the rest
_ABI_SYMBOLS_ROWS = ("lmpc_set_regression_laps_rows", "lmpc_fleet_ss_set_regression_rows")
# the entry points of include/lmpc_hip_cars.h (one plant vehicle per car), resolved at load time in a loop of their own
_ABI_SYMBOLS_CARS = ("lmpc_cars_set_vehicles", "lmpc_cars_get_vehicles", "lmpc_plant_step_cars_batch")
# the entry points of include/lmpc_hip_dtrack.h (the double-track plant), resolved at load time in a loop of their own
_ABI_SYMBOLS_DTRACK = ("lmpc_dtrack_set_vehicles", "lmpc_dtrack_get_vehicles", "lmpc_plant_step_dtrack_batch")
# the entry point of include/lmpc_hip_vanilla_fleet.h (the vanilla rollout of a fleet), resolved at load time in a loop of its own
_ABI_SYMBOLS_VANILLA_FLEET = ("lmpc_vanilla_rollout_fleet_batch",)
# the entry point of include/lmpc_hip_fleet_dtrack.h (the fused fleet LMPC period on the double-track table), in a loop of its own
_ABI_SYMBOLS_FLEET_DTRACK = ("lmpc_fleet_loop_advance_dtrack_batch",)
# the entry points of include/lmpc_hip_dtrack_model.h (the double-track controller model), resolved at load time in a loop of their own
_ABI_SYMBOLS_DTRACK_MODEL = ("lmpc_linearize_dtrack_batch", "lmpc_dtrack_set_controller_model", "lmpc_dtrack_get_controller_model")
# the entry points of include/lmpc_hip_cars_model.h (the per-car single-track controller model), resolved at load time in a loop of their own
_ABI_SYMBOLS_CARS_MODEL = ("lmpc_linearize_cars_batch", "lmpc_cars_set_controller_model", "lmpc_cars_get_controller_model")
# the entry point of include/lmpc_hip_estimated.h (the fused estimated period), resolved at load time in a loop of its own
_ABI_SYMBOLS_ESTIMATED = ("lmpc_loop_advance_estimated_batch",)
VANILLA_PLANT = {"handle": 0, "cars": 1, "dtrack": 2}           # LMPC_VANILLA_PLANT_*
VANILLA_RECORD = {None: 0, "applied": 1, "arrived": 2}          # LMPC_VANILLA_RECORD_*
EKF_FALLBACK, EKF_R_REPAIRED, EKF_NOT_FINITE = 1, 2, 4   # bits of the per-car flags of Solver.ekf_update
LQR_NOT_FINITE = 1   # per-car flag of Solver.lqr_solve: the car's X_optm, U_optm, K or P0 holds a NaN or Inf
VANILLA_NOT_FINITE = 1   # per-car flag of Solver.vanilla_solve / vanilla_rollout: u_out (rollout: or the state after the plant) holds a NaN or Inf


class LmpcError(RuntimeError):
    pass


class CVehicle(C.Structure):
    _fields_ = [("model_id", C.c_int32), ("integrator", C.c_int32)] + [
        (n, C.c_double) for n in
        ("m Jzz l cg_ratio h b fr kd kb cd Af rho cl_f cl_r mu Bf Cf Br Cr Fd_max Fb_max Td Tb "
         "max_steer max_steer_rate").split()]


class CVehicleDT(C.Structure):
    """lmpc_vehicle_dt of include/lmpc_hip_dtrack.h: a CVehicle and the nine doubles of the four-wheel model."""
    _fields_ = [("base", CVehicle)] + [(n, C.c_double) for n in "tw_f tw_r kroll_f Ef Fz0_f eps_f Er Fz0_r eps_r".split()]


class CConfig(C.Structure):
    _fields_ = [("N", C.c_int32), ("learning", C.c_int32), ("num_ss_pts", C.c_int32),
                ("num_ss_pts_per_lap", C.c_int32), ("max_lap_stored", C.c_int32),
                ("max_iter", C.c_int32), ("polish", C.c_int32), ("reserved", C.c_int32),
                ("tol", C.c_double), ("margin", C.c_double),
                ("q_contour", C.c_double), ("q_heading", C.c_double), ("q_vel", C.c_double),
                ("q_vy", C.c_double), ("q_vyaw", C.c_double), ("q_boundary", C.c_double),
                ("R", C.c_double * 4), ("R_d", C.c_double * 4),
                ("x_max", C.c_double * 6), ("x_min", C.c_double * 6),
                ("u_max", C.c_double * 2), ("u_min", C.c_double * 2),
                ("convex_hull_slack", C.c_double * 6), ("max_vel_ref_diff", C.c_double)]


class CRegressionSpec(C.Structure):
    """lmpc_regression_spec: RegQuery's index lists and bandwidth (safe_set.hpp:57-75)."""
    _fields_ = [("n_out", C.c_int32), ("out", C.c_int32 * 6), ("n_in_state", C.c_int32), ("in_state", C.c_int32 * 6),
                ("n_in_ctrl", C.c_int32), ("in_ctrl", C.c_int32 * 2), ("as_written", C.c_int32), ("dist_max", C.c_double)]


class CRegressionRowsSpec(C.Structure):
    """lmpc_regression_rows_spec: RegQuery's index lists, one list per regressed row (safe_set.hpp:61-75), and its bandwidth."""
    _fields_ = [("n_out", C.c_int32), ("out", C.c_int32 * 6), ("n_in_state", C.c_int32 * 6), ("in_state", (C.c_int32 * 6) * 6),
                ("n_in_ctrl", C.c_int32 * 6), ("in_ctrl", (C.c_int32 * 2) * 6), ("as_written", C.c_int32), ("dist_max", C.c_double)]


def _rows_exclude_one_list(rows, in_state, in_ctrl, out_rows):
    """rows= carries its own lists: the one-list keywords must then be at their defaults (None, the fleet method's "off", included)."""
    if rows is not None and not ((in_state is None or tuple(in_state) == (3, 4, 5)) and tuple(in_ctrl) == (0, 1) and tuple(out_rows) == (3, 4, 5)):
        raise ValueError("rows= carries one (in_state, in_ctrl) list per regressed row: in_state=, in_ctrl= and out_rows= go with the one-list form")


def _rows_spec(rows, dist_max, as_written) -> CRegressionRowsSpec:
    """rows: {row: (in_state, in_ctrl), ...} in insertion order -> lmpc_regression_rows_spec.  Sizes the struct cannot hold are refused
    here; everything else is the library's to refuse."""
    rows = list(dict(rows).items())
    if len(rows) > 6 or any(len(s) > 6 or len(c) > 2 for _, (s, c) in rows):
        raise LmpcError("rows=: at most 6 rows of at most 6 feature states and 2 feature controls fit lmpc_regression_rows_spec")
    spec = CRegressionRowsSpec()
    spec.n_out, spec.dist_max, spec.as_written = len(rows), float(dist_max), 1 if as_written else 0
    for o, (r, (ins, inc)) in enumerate(rows):
        spec.out[o], spec.n_in_state[o], spec.n_in_ctrl[o] = int(r), len(ins), len(inc)
        for f, v in enumerate(ins):
            spec.in_state[o][f] = int(v)
        for f, v in enumerate(inc):
            spec.in_ctrl[o][f] = int(v)
    return spec


class CFleetLoop(C.Structure):
    """lmpc_fleet_loop: everything lmpc_fleet_loop_advance_batch takes beside the handle, the batch and the track."""
    _fields_ = ([(n, C.c_void_p) for n in "X_trk U_trk status_trk X_lrn U_lrn status_lrn x u_prev X_ref U_ref T_ref bound_left bound_right "
                                          "curvatures vel_ref".split()]
                + [("dt", C.c_double), ("dt_sim", C.c_double), ("t", C.c_double), ("speed_scale", C.c_double * 2),
                   ("speed_limit", C.c_double * 2), ("max_vel_ref_diff", C.c_double * 2)]
                + [(n, C.c_int32) for n in "n_sub restart_failed warm_laps learn_laps switch_phase n_rec".split()]
                + [("plant", C.POINTER(CVehicle))]
                + [(n, C.c_void_p) for n in "phase n_learn lap_time lap_kind counters x_ic query distance worst_excess n_fail".split()])


class CEstimatedLoop(C.Structure):
    """lmpc_estimated_loop of include/lmpc_hip_estimated.h: everything lmpc_loop_advance_estimated_batch takes beside the handle, the
    batch and the two tracks."""
    _fields_ = ([(n, C.c_void_p) for n in "X_optm U_optm status x u_prev x_ic X_ref U_ref T_ref bound_left bound_right curvatures vel_ref".split()]
                + [(n, C.c_double) for n in "dt dt_sim speed_scale speed_limit".split()]
                + [(n, C.c_int32) for n in "n_sub restart_failed obs_vel obs_pose".split()]
                + [("t_vel_ns", C.c_int64), ("t_pose_ns", C.c_int64)]
                + [(n, C.c_void_p) for n in "noise_vel R_vel noise_pose R_pose x_est z_vel z_pose ekf_flags track_status distance worst_excess "
                                            "n_fail sq_err".split()])


class CEkfConfig(C.Structure):
    """lmpc_ekf_config: the filter's start, process noise and clip (ekf_state_estimator_config.hpp)."""
    _fields_ = [("x0", C.c_double * 6), ("P0", C.c_double * 36), ("Q", C.c_double * 36), ("x_min", C.c_double * 6), ("x_max", C.c_double * 6)]


class CLqrConfig(C.Structure):
    """lmpc_lqr_config: horizon, time step and the three general dense weights, row-major (racing_lqr_config.hpp)."""
    _fields_ = [("N", C.c_int32), ("reserved", C.c_int32), ("dt", C.c_double), ("Q", C.c_double * 36), ("R", C.c_double * 4),
                ("Qf", C.c_double * 36)]


class CVanillaConfig(C.Structure):
    """lmpc_vanilla_config: pure pursuit's lookahead, the PID's coefficients and dt, newtons -> model command
    (vanilla_controller_config.hpp, lmpc_utils/pid_controller.hpp)."""
    _fields_ = [(n, C.c_double) for n in ("lookahead_speed_ratio min_lookahead_distance max_lookahead_distance k_p k_i k_d min_cmd max_cmd "
                                          "min_i max_i dt force_to_lon").split()]


class CVanillaFleetRollout(C.Structure):
    """lmpc_vanilla_fleet_rollout of include/lmpc_hip_vanilla_fleet.h: everything lmpc_vanilla_rollout_fleet_batch takes beside the
    handle, the batch, the spline track and the table."""
    _fields_ = ([("x", C.c_void_p), ("u_prev", C.c_void_p)] + [(n, C.c_int32) for n in "periods n_sub plant record".split()]
                + [("dt_sim", C.c_double), ("speed_scale", C.c_double), ("period0", C.c_int64), ("dt", C.c_double)]
                + [(n, C.c_void_p) for n in "X_log U_log k_log distance worst_excess flags".split()])


class CTrack(C.Structure):
    _fields_ = [("L", C.c_double), ("M", C.c_int32), ("reserved", C.c_int32),
                ("curvature", C.c_void_p), ("bound_left", C.c_void_p), ("bound_right", C.c_void_p),
                ("vel", C.c_void_p)]


def _fill(struct, values: dict):
    for name, ctype in struct._fields_:
        if name == "reserved":
            continue
        if name == "polish":         # 0 (default): on, < 0: off -- presets need not carry the key
            setattr(struct, name, int(values.get("polish", 0)))
            continue
        if name == "integrator":     # modeling.integrator_type, "rk4" (default) or "euler"
            iv = values.get("integrator", 0)
            setattr(struct, name, {"rk4": 0, "euler": 1}[iv] if isinstance(iv, str) else int(iv))
            continue
        v = values[name]
        if hasattr(ctype, "_length_"):
            getattr(struct, name)[:] = [float(a) for a in v]
        elif ctype is C.c_int32:
            setattr(struct, name, int(v))
        else:
            setattr(struct, name, float(v))
    return struct


def library_path() -> Path:
    """The built library; LMPC_HIP_LIBRARY names another build of it (A/B timing of a variant, scratch/)."""
    import os
    return Path(os.environ["LMPC_HIP_LIBRARY"]) if os.environ.get("LMPC_HIP_LIBRARY") else _HERE / "lib" / "liblmpc_hip.so"


def load_library():
    """Load liblmpc_hip.so.  Raises if it has not been built (no CPU fallback exists)."""
    global _LIB
    if _LIB is None:
        so = library_path()
        if not so.exists():
            raise LmpcError(f"{so} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            f"or `make -C {_HERE / 'csrc'}`")
        lib = C.CDLL(str(so))
        for sym in _ABI_SYMBOLS + _ABI_SYMBOLS_ROWS:
            getattr(lib, sym)
        for sym in _ABI_SYMBOLS_CARS:
            getattr(lib, sym)
        for sym in _ABI_SYMBOLS_DTRACK:
            getattr(lib, sym)
        for sym in _ABI_SYMBOLS_VANILLA_FLEET:
            getattr(lib, sym)
        for sym in _ABI_SYMBOLS_FLEET_DTRACK:
            getattr(lib, sym)
        for sym in _ABI_SYMBOLS_DTRACK_MODEL:
            getattr(lib, sym)
        for sym in _ABI_SYMBOLS_CARS_MODEL:
            getattr(lib, sym)
        for sym in _ABI_SYMBOLS_ESTIMATED:
            getattr(lib, sym)
        lib.lmpc_last_error.restype = C.c_char_p
        lib.lmpc_last_error.argtypes = [C.c_void_p]
        lib.lmpc_destroy.restype = None
        lib.lmpc_destroy.argtypes = [C.c_void_p]
        _LIB = lib
    return _LIB


def _ptr(t):
    if t is None:
        return C.c_void_p(0)
    return C.c_void_p(t.data_ptr())


class SplineTrack:
    """A track's splines on the device (lmpc_spline_track), made by Solver.spline_track; freed by close() or with the object."""

    def __init__(self, solver, ptr, L: float, h_bar: float, n_wp: int):
        self._solver, self._p = solver, ptr
        self.L, self.h_bar, self.n_wp = L, h_bar, n_wp

    def close(self):
        if getattr(self, "_p", None) and getattr(self._solver, "_h", None):
            self._solver.lib.lmpc_spline_track_destroy(self._solver._h, self._p)
        self._p = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Solver:
    """Batched RacingMPC on one GPU.  Not re-entrant; one instance per device."""

    def __init__(self, config: dict, vehicle: dict, device: int = 0):
        import torch

        self._torch = torch
        self.lib = load_library()
        self.config = dict(config)
        self.vehicle = dict(vehicle)
        self.N = int(config["N"])
        self.device = torch.device("cuda", device)
        self._h = C.c_void_p(0)
        cc, cv = _fill(CConfig(), config), _fill(CVehicle(), vehicle)
        rc = self.lib.lmpc_create(C.byref(cc), C.byref(cv), C.c_int(device), C.byref(self._h))
        if rc != 0:
            msg = self.lib.lmpc_last_error(self._h).decode() if self._h else "allocation failed"
            if self._h:
                self.lib.lmpc_destroy(self._h)
                self._h = C.c_void_p(0)
            raise LmpcError(f"lmpc_create -> {rc}: {msg}")
        self._track_keepalive = None

    def close(self):
        if getattr(self, "_h", None):
            self.lib.lmpc_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise LmpcError(f"{what} -> {rc}: {self.lib.lmpc_last_error(self._h).decode()}")

    def _t(self, x):
        torch = self._torch
        t = torch.as_tensor(x, dtype=torch.float64, device=self.device)
        return t.contiguous()

    def use_current_stream(self):
        """Queue launches on torch's current stream, so that torch copies, ops and events order
        with the kernels.  Called by every method below before it launches."""
        s = self._torch.cuda.current_stream(self.device).cuda_stream
        if s != getattr(self, "_stream", None):
            self._check(self.lib.lmpc_set_stream(self._h, C.c_void_p(s)), "lmpc_set_stream")
            self._stream = s

    def synchronize(self):
        self._check(self.lib.lmpc_synchronize(self._h), "lmpc_synchronize")

    def reserve(self, max_batch: int):
        self._check(self.lib.lmpc_reserve(self._h, C.c_int32(max_batch)), "lmpc_reserve")

    def enable_timing(self, on: bool = True):
        self._check(self.lib.lmpc_enable_timing(self._h, C.c_int32(int(on))), "lmpc_enable_timing")

    def last_kernel_ms(self):
        a, b = C.c_float(0), C.c_float(0)
        self._check(self.lib.lmpc_last_kernel_ms(self._h, C.byref(a), C.byref(b)), "lmpc_last_kernel_ms")
        return a.value, b.value

    def launch_info(self, precision: str = "f64"):
        """LDS bytes and resident problems per CU of the kernel the given entry point launches ("f64", "f32", "mixed")."""
        a, b = C.c_int32(0), C.c_int32(0)
        self._check(self.lib.lmpc_query_launch(self._h, C.byref(a), C.byref(b)), "lmpc_query_launch")
        c = C.c_int32(0)
        self._check(self.lib.lmpc_query_launch_for(self._h, C.c_int32({"f64": 0, "f32": 1, "mixed": 2}[precision]), C.byref(a), C.byref(c)),
                    "lmpc_query_launch_for")
        return {"lds_bytes_per_problem": a.value, "threads_per_problem": b.value, "resident_problems_per_cu": c.value}

    # ---- input preparation (racing_mpc_node.cpp:210-235,261-292) ----
    def prepare(self, track: dict, x_ic, dt: float, speed_scale: float = 1.0, speed_limit: float | None = None):
        torch = self._torch
        self.use_current_stream()
        x_ic = self._t(x_ic)
        B, N = x_ic.shape[1], self.N
        tabs = {k: self._t(track[k]) for k in ("curvature", "bound_left", "bound_right", "vel")}
        ct = CTrack(float(track["L"]), int(tabs["curvature"].numel()), 0, tabs["curvature"].data_ptr(),
                    tabs["bound_left"].data_ptr(), tabs["bound_right"].data_ptr(), tabs["vel"].data_ptr())
        if speed_limit is None:
            speed_limit = float(self.config["x_max"][3])
        kw = dict(dtype=torch.float64, device=self.device)
        out = {"X_ref": torch.empty((6, N, B), **kw), "U_ref": torch.empty((2, N - 1, B), **kw),
               "T_ref": torch.empty((N - 1, B), **kw), "bound_left": torch.empty((N, B), **kw),
               "bound_right": torch.empty((N, B), **kw), "curvatures": torch.empty((N, B), **kw),
               "vel_ref": torch.empty((N, B), **kw)}
        rc = self.lib.lmpc_prepare_batch(self._h, C.c_int32(B), C.byref(ct), _ptr(x_ic), C.c_double(dt),
                                         C.c_double(speed_scale), C.c_double(speed_limit),
                                         *[_ptr(out[k]) for k in ("X_ref", "U_ref", "T_ref", "bound_left",
                                                                  "bound_right", "curvatures", "vel_ref")])
        self._check(rc, "lmpc_prepare_batch")
        self._track_keepalive = tabs
        out["x_ic"] = x_ic
        out["L"] = float(track["L"])
        return out

    def prepare_failed(self, track: dict, x_ic, status, inp: dict, dt: float, speed_scale: float = 1.0,
                       speed_limit: float | None = None):
        """lmpc_prepare_failed_batch: cold start, in place in `inp`, of the problems with status != 0."""
        self.use_current_stream()
        ct = self._ctrack(track)
        if speed_limit is None:
            speed_limit = float(self.config["x_max"][3])
        x_ic = self._t(x_ic)
        rc = self.lib.lmpc_prepare_failed_batch(self._h, C.c_int32(x_ic.shape[1]), C.byref(ct), _ptr(x_ic), _ptr(status),
                                                C.c_double(dt), C.c_double(speed_scale), C.c_double(speed_limit),
                                                *[_ptr(inp[k]) for k in ("X_ref", "U_ref", "T_ref", "bound_left",
                                                                         "bound_right", "curvatures", "vel_ref")])
        self._check(rc, "lmpc_prepare_failed_batch")
        return inp

    def _ctrack(self, track: dict):
        tabs = {k: self._t(track[k]) for k in ("curvature", "bound_left", "bound_right", "vel")}
        ct = CTrack(float(track["L"]), int(tabs["curvature"].numel()), 0, tabs["curvature"].data_ptr(),
                    tabs["bound_left"].data_ptr(), tabs["bound_right"].data_ptr(), tabs["vel"].data_ptr())
        self._track_keepalive = tabs
        return ct

    def device_track(self, track: dict) -> dict:
        """Upload the track tables once; the returned dict can be passed wherever `track` is expected."""
        out = {k: self._t(track[k]) for k in ("curvature", "bound_left", "bound_right", "vel")}
        out["L"] = float(track["L"])
        out["M"] = int(track["M"])
        return out

    # ---- warm-start shift (racing_mpc_node.cpp:245-254,261-292) ----
    def shift(self, track: dict, prev_inp: dict, sol: dict, dt: float, speed_scale: float = 1.0,
              speed_limit: float | None = None):
        torch = self._torch
        self.use_current_stream()
        ct = self._ctrack(track)
        N = self.N
        B = sol["X_optm"].shape[2]
        if speed_limit is None:
            speed_limit = float(self.config["x_max"][3])
        kw = dict(dtype=torch.float64, device=self.device)
        out = {"X_ref": torch.empty((6, N, B), **kw), "U_ref": torch.empty((2, N - 1, B), **kw),
               "T_ref": torch.empty((N - 1, B), **kw), "bound_left": torch.empty((N, B), **kw),
               "bound_right": torch.empty((N, B), **kw), "curvatures": torch.empty((N, B), **kw),
               "vel_ref": torch.empty((N, B), **kw), "L": float(track["L"])}
        rc = self.lib.lmpc_shift_batch(self._h, C.c_int32(B), C.byref(ct), _ptr(sol["X_optm"]), _ptr(sol["U_optm"]),
                                       _ptr(prev_inp["X_ref"]), _ptr(prev_inp["U_ref"]), _ptr(sol["status"]),
                                       C.c_double(dt), C.c_double(speed_scale), C.c_double(speed_limit),
                                       *[_ptr(out[k]) for k in ("X_ref", "U_ref", "T_ref", "bound_left",
                                                                "bound_right", "curvatures", "vel_ref")])
        self._check(rc, "lmpc_shift_batch")
        return out

    def set_output_layout(self, layout: str = "soa"):
        """"soa": results [component][knot][batch] (default); "aos": [batch][knot][component] (include/lmpc_hip.h).  The caller
        passes result tensors of the matching shape (alloc_outputs follows the setting)."""
        self._aos = {"soa": False, "aos": True}[layout]
        self._check(self.lib.lmpc_set_output_layout(self._h, C.c_int32(int(self._aos))), "lmpc_set_output_layout")

    def set_warm_rounds(self, rounds: int = 0):
        """Repair rounds a warm start may spend before the cold start takes over (include/lmpc_hip.h): 1 .. 4, or 0 for the default
        (2 rounds; 4 when the batch is at least four times what the device holds at once)."""
        self._check(self.lib.lmpc_set_warm_rounds(self._h, C.c_int32(int(rounds))), "lmpc_set_warm_rounds")

    # ---- launch order (longest job first; include/lmpc_hip.h) ----
    def set_launch_order(self, order):
        """order: int32 device tensor [batch] (kept alive here; applies to solves of that batch size) or None for the default mapping."""
        self._launch_order = None if order is None else self._torch.as_tensor(order, dtype=self._torch.int32, device=self.device).contiguous()
        n = 0 if self._launch_order is None else int(self._launch_order.numel())
        self._check(self.lib.lmpc_set_launch_order(self._h, _ptr(self._launch_order), C.c_int32(n)), "lmpc_set_launch_order")

    def launch_order_from_iters(self, iters, order=None):
        """Fills (and returns) `order` from the iteration counts of the previous solve of the same batch, longest first."""
        torch = self._torch
        self.use_current_stream()
        iters = torch.as_tensor(iters, dtype=torch.int32, device=self.device).contiguous()
        if order is None:
            order = torch.empty_like(iters)
        self._check(self.lib.lmpc_launch_order_from_iters(self._h, C.c_int32(iters.numel()), _ptr(iters), _ptr(order)),
                    "lmpc_launch_order_from_iters")
        return order

    # ---- plant (racing_simulator.cpp:97-112) ----
    def plant_step(self, track: dict, x, u, dt_sim: float, n_sub: int = 1):
        self.use_current_stream()
        ct = self._ctrack(track)
        rc = self.lib.lmpc_plant_step_batch(self._h, C.c_int32(x.shape[1]), C.byref(ct), _ptr(x), _ptr(u),
                                            C.c_double(dt_sim), C.c_int32(n_sub))
        self._check(rc, "lmpc_plant_step_batch")
        return x

    # ---- one plant vehicle per car (include/lmpc_hip_cars.h) ----
    def set_car_vehicles(self, vehicles):
        """lmpc_cars_set_vehicles: a sequence of B vehicle dicts (the keys of this solver's `vehicle`; "integrator" "rk4" | "euler" per
        car) becomes the handle's car table; None or an empty sequence switches it off.  While it is set, plant_step_cars steps car b
        with vehicle b and so does fleet_loop_advance, which then refuses plant= and any batch but B.  Blocking."""
        self.use_current_stream()
        vehicles = list(vehicles) if vehicles is not None else []
        if not vehicles:
            self._check(self.lib.lmpc_cars_set_vehicles(self._h, C.c_int32(0), C.c_void_p(0)), "lmpc_cars_set_vehicles")
            self._n_cars = 0
            return
        arr = (CVehicle * len(vehicles))()
        filled = {}   # a dict that stands for many cars (a fleet of a few kinds) is converted once
        for b, v in enumerate(vehicles):
            if id(v) not in filled:
                filled[id(v)] = _fill(CVehicle(), v)
            arr[b] = filled[id(v)]
        self._check(self.lib.lmpc_cars_set_vehicles(self._h, C.c_int32(len(vehicles)), arr), "lmpc_cars_set_vehicles")
        self._n_cars = len(vehicles)   # (a refused call has raised: the table in effect before it, and its size, stay)

    def car_vehicles(self):
        """lmpc_cars_get_vehicles: the car table read back, a list of B vehicle dicts ("integrator" as 0 | 1).  Blocking; refused
        without a table."""
        self.use_current_stream()
        n = getattr(self, "_n_cars", 0)
        arr = (CVehicle * max(n, 1))()
        self._check(self.lib.lmpc_cars_get_vehicles(self._h, C.c_int32(n), arr), "lmpc_cars_get_vehicles")
        return [{name: getattr(cv, name) for name, _ in CVehicle._fields_} for cv in arr[:n]]

    def plant_step_cars(self, track: dict, x, u, dt_sim: float, n_sub: int = 1):
        """lmpc_plant_step_cars_batch: plant_step with car b stepped by vehicle b of the car table."""
        self.use_current_stream()
        ct = self._ctrack(track)
        rc = self.lib.lmpc_plant_step_cars_batch(self._h, C.c_int32(x.shape[1]), C.byref(ct), _ptr(x), _ptr(u),
                                                 C.c_double(dt_sim), C.c_int32(n_sub))
        self._check(rc, "lmpc_plant_step_cars_batch")
        return x

    # ---- the double-track plant: one four-wheel vehicle per car (include/lmpc_hip_dtrack.h) ----
    def set_dtrack_vehicles(self, vehicles):
        """lmpc_dtrack_set_vehicles: a sequence of B double-track vehicle dicts (presets.barc_double_track's keys: the vehicle's, with
        model_id 2, and tw_f, tw_r, kroll_f, Ef, Fz0_f, eps_f, Er, Fz0_r, eps_r; "integrator" "rk4" | "euler" per car) becomes the
        handle's double-track table; None or an empty sequence switches it off.  plant_step_dtrack reads it, vanilla_rollout_fleet(plant="dtrack") and
        fleet_loop_advance(dtrack=True).  Blocking."""
        self.use_current_stream()
        vehicles = list(vehicles) if vehicles is not None else []
        if not vehicles:
            self._check(self.lib.lmpc_dtrack_set_vehicles(self._h, C.c_int32(0), C.c_void_p(0)), "lmpc_dtrack_set_vehicles")
            self._n_dtrack = 0
            return
        arr = (CVehicleDT * len(vehicles))()
        filled = {}   # a dict that stands for many cars (a fleet of a few kinds) is converted once
        for b, v in enumerate(vehicles):
            if id(v) not in filled:
                cv = CVehicleDT()
                _fill(cv.base, v)
                for name, _ in CVehicleDT._fields_[1:]:
                    setattr(cv, name, float(v[name]))
                filled[id(v)] = cv
            arr[b] = filled[id(v)]
        self._check(self.lib.lmpc_dtrack_set_vehicles(self._h, C.c_int32(len(vehicles)), arr), "lmpc_dtrack_set_vehicles")
        self._n_dtrack = len(vehicles)   # (a refused call has raised: the table in effect before it, and its size, stay)

    def get_dtrack_vehicles(self):
        """lmpc_dtrack_get_vehicles: the double-track table read back, a list of B flat vehicle dicts ("integrator" as 0 | 1).
        Blocking; refused without a table."""
        self.use_current_stream()
        n = getattr(self, "_n_dtrack", 0)
        arr = (CVehicleDT * max(n, 1))()
        self._check(self.lib.lmpc_dtrack_get_vehicles(self._h, C.c_int32(n), arr), "lmpc_dtrack_get_vehicles")
        return [dict({name: getattr(cv.base, name) for name, _ in CVehicle._fields_},
                     **{name: getattr(cv, name) for name, _ in CVehicleDT._fields_[1:]}) for cv in arr[:n]]

    def plant_step_dtrack(self, track: dict, x, u, dt_sim: float, n_sub: int = 1, gamma_y=None):
        """lmpc_plant_step_dtrack_batch: x [6, B] = [s, e_y, e_psi, vx, vy, omega] advanced in place on the double-track model, car b
        with vehicle b of the double-track table; gamma_y (a float64 [B] tensor, optional) receives the lateral load transfer solved
        in the first evaluation of the last sub-step."""
        self.use_current_stream()
        ct = self._ctrack(track)
        rc = self.lib.lmpc_plant_step_dtrack_batch(self._h, C.c_int32(x.shape[1]), C.byref(ct), _ptr(x), _ptr(u),
                                                   C.c_double(dt_sim), C.c_int32(n_sub), _ptr(gamma_y))
        self._check(rc, "lmpc_plant_step_dtrack_batch")
        return x

    def loop_advance(self, track: dict, inp: dict, sol: dict, x, u_prev, dt: float, dt_sim: float, n_sub: int = 1, speed_scale: float = 1.0,
                     speed_limit: float | None = None, restart_failed: bool = True, distance=None, worst_excess=None, n_fail=None,
                     n_accepted=None):
        """lmpc_loop_advance_batch: input selection + plant step + the next period's inputs (shift, or cold restart of failed cars) +
        bookkeeping in one launch.  `inp`'s reference arrays, `x` [6][B] and `u_prev` [2][B] are updated in place; the accumulators
        (float64 [B], float64 [B], int64 [B], int64 scalar tensor) are optional."""
        self.use_current_stream()
        ct = self._ctrack(track)
        if speed_limit is None:
            speed_limit = float(self.config["x_max"][3])
        rc = self.lib.lmpc_loop_advance_batch(
            self._h, C.c_int32(x.shape[1]), C.byref(ct), _ptr(sol["status"]), _ptr(sol["iters"]), _ptr(sol["X_optm"]), _ptr(sol["U_optm"]),
            _ptr(x), _ptr(u_prev), C.c_double(dt), C.c_double(dt_sim), C.c_int32(n_sub), C.c_double(speed_scale), C.c_double(speed_limit),
            C.c_int32(1 if restart_failed else 0), *[_ptr(inp[k]) for k in ("X_ref", "U_ref", "T_ref", "bound_left", "bound_right", "curvatures", "vel_ref")],
            _ptr(distance), _ptr(worst_excess), _ptr(n_fail), _ptr(n_accepted))
        self._check(rc, "lmpc_loop_advance_batch")

    # ---- discrete_dynamics_jacobian (single_track_planar_model.cpp:377-387) ----
    def linearize(self, inp: dict):
        torch = self._torch
        self.use_current_stream()
        X, U, T, kap = (self._t(inp[k]) for k in ("X_ref", "U_ref", "T_ref", "curvatures"))
        B, N = X.shape[2], self.N
        kw = dict(dtype=torch.float64, device=self.device)
        A = torch.empty((6, 6, N - 1, B), **kw)
        Bm = torch.empty((6, 2, N - 1, B), **kw)
        g = torch.empty((6, N - 1, B), **kw)
        rc = self.lib.lmpc_linearize_batch(self._h, C.c_int32(B), _ptr(X), _ptr(U), _ptr(T), _ptr(kap), _ptr(A),
                                           _ptr(Bm), _ptr(g))
        self._check(rc, "lmpc_linearize_batch")
        return A, Bm, g

    # ---- the double-track controller model (include/lmpc_hip_dtrack_model.h) ----
    def linearize_dtrack(self, inp: dict, out=None):
        """lmpc_linearize_dtrack_batch: what linearize returns -- A [6, 6, N-1, B], Bm [6, 2, N-1, B], g [6, N-1, B] -- on the
        double-track model, problem b on vehicle b of the double-track table (set_dtrack_vehicles).  `out`: an (A, Bm, g) of float64
        tensors to write into instead of fresh ones.  Asynchronous; refused without a table or with a batch other than the table's."""
        torch = self._torch
        self.use_current_stream()
        X, U, T, kap = (self._t(inp[k]) for k in ("X_ref", "U_ref", "T_ref", "curvatures"))
        B, N = X.shape[2], self.N
        kw = dict(dtype=torch.float64, device=self.device)
        A, Bm, g = out if out is not None else (torch.empty((6, 6, N - 1, B), **kw), torch.empty((6, 2, N - 1, B), **kw),
                                                torch.empty((6, N - 1, B), **kw))
        rc = self.lib.lmpc_linearize_dtrack_batch(self._h, C.c_int32(B), _ptr(X), _ptr(U), _ptr(T), _ptr(kap), _ptr(A), _ptr(Bm), _ptr(g))
        self._check(rc, "lmpc_linearize_dtrack_batch")
        return A, Bm, g

    def set_dtrack_controller_model(self, on: bool):
        """lmpc_dtrack_set_controller_model: while on, solve(...) -- fp64, mixed, warm, with the safe set as arrays or by reference --
        linearises problem b on vehicle b of the double-track table and must be given the table's batch; solve_f32 and the
        sequential-QP solve are refused.  Needs a table; refused while a regression is in effect.  Host-only."""
        self._check(self.lib.lmpc_dtrack_set_controller_model(self._h, C.c_int32(1 if on else 0)), "lmpc_dtrack_set_controller_model")

    @property
    def dtrack_controller_model(self) -> bool:
        """lmpc_dtrack_get_controller_model: whether the solves run on the double-track model."""
        on = C.c_int32(0)
        self._check(self.lib.lmpc_dtrack_get_controller_model(self._h, C.byref(on)), "lmpc_dtrack_get_controller_model")
        return bool(on.value)

    # ---- the per-car single-track controller model (include/lmpc_hip_cars_model.h) ----
    def linearize_cars(self, inp: dict, out=None):
        """lmpc_linearize_cars_batch: what linearize returns -- A [6, 6, N-1, B], Bm [6, 2, N-1, B], g [6, N-1, B] -- with problem b
        linearised on vehicle b of the car table (set_car_vehicles).  `out`: an (A, Bm, g) of float64 tensors to write into instead of
        fresh ones.  Asynchronous; refused without a table or with a batch other than the table's."""
        torch = self._torch
        self.use_current_stream()
        X, U, T, kap = (self._t(inp[k]) for k in ("X_ref", "U_ref", "T_ref", "curvatures"))
        B, N = X.shape[2], self.N
        kw = dict(dtype=torch.float64, device=self.device)
        A, Bm, g = out if out is not None else (torch.empty((6, 6, N - 1, B), **kw), torch.empty((6, 2, N - 1, B), **kw),
                                                torch.empty((6, N - 1, B), **kw))
        rc = self.lib.lmpc_linearize_cars_batch(self._h, C.c_int32(B), _ptr(X), _ptr(U), _ptr(T), _ptr(kap), _ptr(A), _ptr(Bm), _ptr(g))
        self._check(rc, "lmpc_linearize_cars_batch")
        return A, Bm, g

    def set_cars_controller_model(self, on: bool):
        """lmpc_cars_set_controller_model: while on, solve(...) -- fp64, mixed, warm, with the safe set as arrays or by reference --
        and solve_f32 linearise problem b on vehicle b of the car table and must be given the table's batch; the sequential-QP solve
        is refused.  Needs a table; refused while a regression or the double-track controller model is in effect.  Host-only."""
        self._check(self.lib.lmpc_cars_set_controller_model(self._h, C.c_int32(1 if on else 0)), "lmpc_cars_set_controller_model")

    @property
    def cars_controller_model(self) -> bool:
        """lmpc_cars_get_controller_model: whether the solves linearise each problem on its car's vehicle."""
        on = C.c_int32(0)
        self._check(self.lib.lmpc_cars_get_controller_model(self._h, C.byref(on)), "lmpc_cars_get_controller_model")
        return bool(on.value)

    # ---- RacingMPC::solve (racing_mpc.cpp:209-372) ----
    def alloc_outputs(self, B: int, aos: bool | None = None):
        """Result tensors for a batch of B in the layout lmpc_solve_batch / _mixed write (set_output_layout), or, with
        aos=False, in the default layout whatever the setting (what every other entry point writes)."""
        torch = self._torch
        N = self.N
        kw = dict(dtype=torch.float64, device=self.device)
        if aos is None:
            aos = getattr(self, "_aos", False)
        shapes = ((B, N, 6), (B, N - 1, 2)) if aos else ((6, N, B), (2, N - 1, B))
        return {"X_optm": torch.empty(shapes[0], **kw), "U_optm": torch.empty(shapes[1], **kw),
                "dU_optm": torch.empty(shapes[1], **kw),
                "status": torch.empty((B,), dtype=torch.int32, device=self.device),
                "iters": torch.empty((B,), dtype=torch.int32, device=self.device),
                "kkt": torch.empty((4, B), **kw)}

    def solve(self, inp: dict, out: dict | None = None, ss_x=None, ss_j=None, mixed: bool = False, ss_idx=None, warm=None):
        """lmpc_solve_batch, or with mixed=True lmpc_solve_batch_mixed (same fp64 arrays, fp32 interior-point iteration); with
        ss_idx (int32 [S][B] from ss_query_idx) lmpc_solve_batch_ss_idx: the safe set by reference instead of ss_x / ss_j."""
        self.use_current_stream()
        keys = ("x_ic", "u_ic", "X_ref", "U_ref", "T_ref", "bound_left", "bound_right", "curvatures", "vel_ref")
        a = [self._t(inp[k]) for k in keys]
        B = a[0].shape[1]
        if out is None:
            out = self.alloc_outputs(B)
        if warm is not None and mixed:
            # (this combination used to run the fp64 warm solve and say nothing)
            raise ValueError("Solver.solve: warm start and mixed precision do not combine (lmpc_solve_batch_warm is the fp64 entry)")
        if warm is not None and bool(self.config["learning"]):
            # lmpc_solve_batch_warm_ss: the plan AND its simplex weights (convex_combi_optm_ref, aligned with this call's points)
            wx = a[2] if warm is True else self._t(warm["X_optm_ref"])
            wu = a[3] if warm is True else self._t(warm["U_optm_ref"])
            wl = None if warm is True or warm.get("convex_combi_optm_ref") is None else self._t(warm["convex_combi_optm_ref"])
            sx = None if (ss_x is None or ss_idx is not None) else self._t(ss_x)
            sj = None if (ss_j is None or ss_idx is not None) else self._t(ss_j)
            rc = self.lib.lmpc_solve_batch_warm_ss(self._h, C.c_int32(B), *[_ptr(t) for t in a], C.c_double(float(inp["L"])), _ptr(sx), _ptr(sj),
                                                   _ptr(ss_idx), _ptr(wx), _ptr(wu), _ptr(wl), _ptr(out["X_optm"]), _ptr(out["U_optm"]),
                                                   _ptr(out["dU_optm"]), _ptr(out.get("convex_combi_optm")), _ptr(out["status"]), _ptr(out["iters"]),
                                                   _ptr(out.get("kkt")))
            self._check(rc, "lmpc_solve_batch_warm_ss")
            out["_inputs_keepalive"] = a + [wx, wu, wl, sx, sj, ss_idx]
            return out
        if warm is not None and ss_idx is not None:
            raise ValueError("Solver.solve: ss_idx goes with a learning handle")
        if warm is not None:
            # lmpc_solve_batch_warm: warm = True takes (X_ref, U_ref) as the plan (what the node does), or a dict with X_optm_ref / U_optm_ref
            wx = a[2] if warm is True else self._t(warm["X_optm_ref"])
            wu = a[3] if warm is True else self._t(warm["U_optm_ref"])
            rc = self.lib.lmpc_solve_batch_warm(self._h, C.c_int32(B), *[_ptr(t) for t in a], C.c_double(float(inp["L"])), _ptr(wx), _ptr(wu),
                                                _ptr(out["X_optm"]), _ptr(out["U_optm"]), _ptr(out["dU_optm"]), _ptr(out["status"]),
                                                _ptr(out["iters"]), _ptr(out.get("kkt")))
            self._check(rc, "lmpc_solve_batch_warm")
            out["_inputs_keepalive"] = a + [wx, wu]
            return out
        if ss_idx is not None:
            rc = self.lib.lmpc_solve_batch_ss_idx(self._h, C.c_int32(B), C.c_int32(2 if mixed else 0), *[_ptr(t) for t in a],
                                                  C.c_double(float(inp["L"])), _ptr(ss_idx), _ptr(out["X_optm"]), _ptr(out["U_optm"]),
                                                  _ptr(out["dU_optm"]), _ptr(out.get("convex_combi_optm")), _ptr(out["status"]),
                                                  _ptr(out["iters"]), _ptr(out.get("kkt")))
            self._check(rc, "lmpc_solve_batch_ss_idx")
            out["_inputs_keepalive"] = a + [ss_idx]
            return out
        ss_x = None if ss_x is None else self._t(ss_x)
        ss_j = None if ss_j is None else self._t(ss_j)
        fn = self.lib.lmpc_solve_batch_mixed if mixed else self.lib.lmpc_solve_batch
        rc = fn(self._h, C.c_int32(B), *[_ptr(t) for t in a], C.c_double(float(inp["L"])),
                _ptr(ss_x), _ptr(ss_j), _ptr(out["X_optm"]), _ptr(out["U_optm"]),
                _ptr(out["dU_optm"]), _ptr(out.get("convex_combi_optm")),
                _ptr(out["status"]), _ptr(out["iters"]), _ptr(out.get("kkt")))
        self._check(rc, "lmpc_solve_batch_mixed" if mixed else "lmpc_solve_batch")
        out["_inputs_keepalive"] = a
        return out

    def shift_lambda(self, idx_prev, lam_prev, idx, advance: int = 1, out=None):
        """lmpc_shift_lambda_batch: the previous solution's simplex weights carried onto this period's safe-set codes."""
        torch = self._torch
        self.use_current_stream()
        S, B = idx.shape
        if out is None:
            out = torch.empty((S, B), dtype=torch.float64, device=self.device)
        self._check(self.lib.lmpc_shift_lambda_batch(self._h, C.c_int32(B), _ptr(idx_prev), _ptr(lam_prev), _ptr(idx), C.c_int32(int(advance)), _ptr(out)),
                    "lmpc_shift_lambda_batch")
        return out

    def warm_accepted(self, B: int, out=None):
        """lmpc_get_warm_accepted: int32 [B], 1 where the last warm solve's active-set attempt was accepted."""
        torch = self._torch
        self.use_current_stream()
        if out is None:
            out = torch.empty((B,), dtype=torch.int32, device=self.device)
        self._check(self.lib.lmpc_get_warm_accepted(self._h, C.c_int32(B), _ptr(out)), "lmpc_get_warm_accepted")
        return out

    def set_waves_per_problem(self, waves: int):
        """lmpc_set_waves_per_problem: 0 the library's choice, 1 / 2 wavefronts per problem (2: fp64 tracking, N >= 24, cold solves)."""
        self._check(self.lib.lmpc_set_waves_per_problem(self._h, C.c_int32(int(waves))), "lmpc_set_waves_per_problem")

    def last_solve_precision(self) -> str:
        """lmpc_last_solve_precision: "f64", "f32" or "mixed" -- what the most recent batched solve ran in (solve(mixed=True) falls
        back to fp64 where no reduced-precision kernel exists for this (N, num_ss_pts): include/lmpc_hip.h)."""
        p = C.c_int32(-1)
        self._check(self.lib.lmpc_last_solve_precision(self._h, C.byref(p)), "lmpc_last_solve_precision")
        return {0: "f64", 1: "f32", 2: "mixed"}[p.value]

    # ---- single precision (BASELINE configs[3]) ----
    def solve_f32(self, inp: dict, out: dict | None = None):
        """lmpc_solve_batch_f32: every array in float32 (inputs are converted if they are not), tracking problem only."""
        torch = self._torch
        self.use_current_stream()
        keys = ("x_ic", "u_ic", "X_ref", "U_ref", "T_ref", "bound_left", "bound_right", "curvatures", "vel_ref")
        a = [torch.as_tensor(inp[k], device=self.device).to(torch.float32).contiguous() for k in keys]
        B, N = a[0].shape[1], self.N
        if out is None:
            kw = dict(dtype=torch.float32, device=self.device)
            # (always the default layout: lmpc_set_output_layout applies to lmpc_solve_batch / _mixed only -- include/lmpc_hip.h --
            # and until round 5 this allocated [B][N][6] under the AOS setting for a kernel that writes [6][N][B]: ADVICE r4)
            shapes = ((6, N, B), (2, N - 1, B))
            out = {"X_optm": torch.empty(shapes[0], **kw), "U_optm": torch.empty(shapes[1], **kw),
                   "dU_optm": torch.empty(shapes[1], **kw), "kkt": torch.empty((4, B), **kw),
                   "status": torch.empty((B,), dtype=torch.int32, device=self.device),
                   "iters": torch.empty((B,), dtype=torch.int32, device=self.device)}
        rc = self.lib.lmpc_solve_batch_f32(self._h, C.c_int32(B), *[_ptr(t) for t in a], _ptr(out["X_optm"]),
                                           _ptr(out["U_optm"]), _ptr(out["dU_optm"]), _ptr(out["status"]),
                                           _ptr(out["iters"]), _ptr(out.get("kkt")))
        self._check(rc, "lmpc_solve_batch_f32")
        out["_inputs_keepalive"] = a
        return out

    # ---- full_dynamics = true (racing_mpc.cpp:162-166; IPOPT upstream, racing_mpc_node.cpp:299-314) ----
    def solve_full_dynamics(self, inp: dict, max_sqp: int = 10, tol: float = 1e-9, ss_x=None, ss_j=None):
        """lmpc_solve_full_dynamics_batch: the nonlinear-dynamics problem x_{i+1} = f_d(x_i, u_i, k_i, t_i) by sequential
        QPs over the same kernels with a line search on the l1 merit function (csrc/lmpc_sqp_kernel.hip); the per-knot
        parameters -- curvature, bounds, vel_ref -- stay fixed, as they are parameters of the reference's NLP too.
        Problems whose QP fails keep their last iterate and report that QP's status.  Returns the iterate reached plus
        "sqp_iters" [B], "sqp_move" [B] (scaled size of the last step) and "defect" [B] (scaled dynamics defect)."""
        torch = self._torch
        self.use_current_stream()
        a = {k: self._t(inp[k]) for k in ("x_ic", "u_ic", "X_ref", "U_ref", "T_ref", "bound_left", "bound_right",
                                          "curvatures", "vel_ref")}
        B = a["x_ic"].shape[1]
        out = self.alloc_outputs(B, aos=False)   # (the output layout setting applies to lmpc_solve_batch / _mixed only)
        kw = dict(device=self.device)
        out["sqp_iters"] = torch.zeros((B,), dtype=torch.int32, **kw)
        out["sqp_move"] = torch.zeros((B,), dtype=torch.float64, **kw)
        out["defect"] = torch.zeros((B,), dtype=torch.float64, **kw)
        learning = bool(self.config["learning"])
        if learning:
            out["convex_combi_optm"] = torch.zeros((int(self.config["num_ss_pts"]), B), dtype=torch.float64, **kw)
            ss_x, ss_j = (None if t is None else self._t(t) for t in (ss_x, ss_j))   # (None: the library refuses the call)
        rc = self.lib.lmpc_solve_full_dynamics_batch(
            self._h, C.c_int32(B), *[_ptr(a[k]) for k in ("x_ic", "u_ic", "X_ref", "U_ref", "T_ref", "bound_left",
                                                           "bound_right", "curvatures", "vel_ref")],
            C.c_double(float(inp.get("L", 0.0))), _ptr(ss_x) if learning else None, _ptr(ss_j) if learning else None,
            C.c_int32(int(max_sqp)), C.c_double(float(tol)), _ptr(out["X_optm"]), _ptr(out["U_optm"]), _ptr(out["dU_optm"]),
            _ptr(out["convex_combi_optm"]) if learning else None, _ptr(out["status"]), _ptr(out["iters"]),
            _ptr(out["sqp_iters"]), _ptr(out["sqp_move"]), _ptr(out["defect"]))
        self._check(rc, "lmpc_solve_full_dynamics_batch")
        out["_inputs_keepalive"] = a
        return out

    def solve_full_dynamics_host(self, inp: dict, b: int = 0, max_sqp: int = 10, tol: float = 1e-9, ss_x=None, ss_j=None) -> dict:
        """lmpc_solve_full_dynamics_host on problem `b` of batched numpy inputs ([field][knot][batch], ss_x [6][S][batch]): ONE
        problem through HOST arrays in the reference's column-major layout, as the facade calls it.  Returns numpy results in the
        batch = 1 device layout (X_optm [6][N][1], ...), so that they compare with a row of solve_full_dynamics."""
        import numpy as np

        N, S = self.N, int(self.config["num_ss_pts"]) if bool(self.config["learning"]) else 0
        col = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64)[..., b].T)      # [field][knot] -> knot-major
        a = [col(inp[k]) for k in ("x_ic", "u_ic", "X_ref", "U_ref", "T_ref", "bound_left", "bound_right", "curvatures", "vel_ref")]
        sx, sj = (None if t is None else col(t) for t in (ss_x, ss_j))
        X, U, dU, lam = np.zeros((N, 6)), np.zeros((N - 1, 2)), np.zeros((N - 1, 2)), np.zeros(max(S, 1))
        ints, dbl = np.zeros(3, dtype=np.int32), np.zeros(2)
        p = lambda t, off=0: C.c_void_p(None if t is None else t.ctypes.data + off * t.itemsize)
        rc = self.lib.lmpc_solve_full_dynamics_host(
            self._h, *[p(t) for t in a], C.c_double(float(inp.get("L", 0.0))), p(sx), p(sj), C.c_int32(int(max_sqp)), C.c_double(float(tol)),
            p(X), p(U), p(dU), p(lam if S else None), p(ints), p(ints, 1), p(ints, 2), p(dbl), p(dbl, 1))
        self._check(rc, "lmpc_solve_full_dynamics_host")
        out = {"X_optm": X.T[:, :, None].copy(), "U_optm": U.T[:, :, None].copy(), "dU_optm": dU.T[:, :, None].copy(),
               "status": ints[0:1].copy(), "iters": ints[1:2].copy(), "sqp_iters": ints[2:3].copy(), "sqp_move": dbl[0:1].copy(),
               "defect": dbl[1:2].copy()}
        if S:
            out["convex_combi_optm"] = lam[:, None].copy()
        return out

    # ---- safe set (safe_set.cpp:116-180) ----
    def set_safe_set(self, laps_x, total_length: float):
        import numpy as np

        n_pts = np.array([np.asarray(a).shape[0] for a in laps_x], dtype=np.int32)
        x = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1, 6) for a in laps_x], 0)) \
            if len(laps_x) else np.zeros((0, 6))
        rc = self.lib.lmpc_set_safe_set(self._h, C.c_int32(len(laps_x)), n_pts.ctypes.data_as(C.c_void_p),
                                        x.ctypes.data_as(C.c_void_p), C.c_double(total_length))
        self._check(rc, "lmpc_set_safe_set")

    # ---- error-dynamics regression (safe_set.cpp:56-114, 182-245) ----
    def set_regression_laps(self, laps, in_state=(3, 4, 5), in_ctrl=(0, 1), out_rows=(3, 4, 5), dist_max: float = 1.0,
                            as_written: bool = False, rows=None):
        """laps: list of (x [n,6], u [n,2], k [n], t [n]) host arrays; an empty list switches the regression off.
        in_state, in_ctrl, out_rows: one feature list for all regressed rows.
        rows = {row: (in_state, in_ctrl), ...}: one feature list per regressed row instead (lmpc_set_regression_laps_rows), in
        insertion order; the three one-list keywords then stay at their defaults.
        as_written = True reproduces the reference's literal signs (backward time step, b = -M'K y; lmpc_hip.h)."""
        import numpy as np

        _rows_exclude_one_list(rows, in_state, in_ctrl, out_rows)
        if not laps:
            self._check(self.lib.lmpc_set_regression_laps(self._h, C.c_int32(0), None, None, None, None, None, None),
                        "lmpc_set_regression_laps")
            return
        n_pts = np.array([np.asarray(l[0]).shape[0] for l in laps], dtype=np.int32)
        cat = [np.ascontiguousarray(np.concatenate([np.asarray(l[i], dtype=np.float64).reshape(n, -1) for l, n in zip(laps, n_pts)], 0))
               for i in range(4)]
        if rows is not None:
            spec = _rows_spec(rows, dist_max, as_written)
            rc = self.lib.lmpc_set_regression_laps_rows(self._h, C.c_int32(len(laps)), n_pts.ctypes.data_as(C.c_void_p),
                                                        *[a.ctypes.data_as(C.c_void_p) for a in cat], C.byref(spec))
            self._check(rc, "lmpc_set_regression_laps_rows")
            return
        spec = CRegressionSpec()
        spec.n_out, spec.n_in_state, spec.n_in_ctrl, spec.dist_max = len(out_rows), len(in_state), len(in_ctrl), float(dist_max)
        spec.out[:len(out_rows)] = list(out_rows)
        spec.in_state[:len(in_state)] = list(in_state)
        spec.in_ctrl[:len(in_ctrl)] = list(in_ctrl)
        spec.as_written = 1 if as_written else 0
        rc = self.lib.lmpc_set_regression_laps(self._h, C.c_int32(len(laps)), n_pts.ctypes.data_as(C.c_void_p),
                                               *[a.ctypes.data_as(C.c_void_p) for a in cat], C.byref(spec))
        self._check(rc, "lmpc_set_regression_laps")

    def regress(self, inp: dict, A, Bm, g):
        """Adds RegResult onto A [6,6,N-1,B], Bm [6,2,N-1,B], g [6,N-1,B] (device tensors, in place)."""
        self.use_current_stream()
        X, U = self._t(inp["X_ref"]), self._t(inp["U_ref"])
        rc = self.lib.lmpc_regress_batch(self._h, C.c_int32(X.shape[2]), _ptr(X), _ptr(U), _ptr(A), _ptr(Bm), _ptr(g))
        self._check(rc, "lmpc_regress_batch")
        return A, Bm, g

    def ss_query_idx(self, query, out=None):
        """lmpc_ss_query_idx_batch: the safe set of every query by reference -- (ss_idx int32 [S][B], n_found [B]); `out` reuses buffers."""
        torch = self._torch
        self.use_current_stream()
        q = self._t(query)
        B = q.shape[1]
        S = int(self.config["num_ss_pts"])
        if out is not None:
            ss_idx, nf = out
        else:
            ss_idx = torch.full((S, B), -1, dtype=torch.int32, device=self.device)
            nf = torch.zeros((B,), dtype=torch.int32, device=self.device)
        rc = self.lib.lmpc_ss_query_idx_batch(self._h, C.c_int32(B), _ptr(q), _ptr(ss_idx), _ptr(nf))
        self._check(rc, "lmpc_ss_query_idx_batch")
        return ss_idx, nf

    def ss_query(self, query, out=None):
        """lmpc_ss_query_batch.  `out` = (ss_x [6][S][B], ss_j [S][B], n_found [B]) reuses the caller's buffers (the
        kernel writes every entry of a query that found at least one point); otherwise zero-filled ones are allocated."""
        torch = self._torch
        self.use_current_stream()
        q = self._t(query)
        B = q.shape[1]
        S = int(self.config["num_ss_pts"])
        kw = dict(dtype=torch.float64, device=self.device)
        if out is not None:
            ss_x, ss_j, nf = out
        else:
            ss_x = torch.zeros((6, S, B), **kw)
            ss_j = torch.zeros((S, B), **kw)
            nf = torch.zeros((B,), dtype=torch.int32, device=self.device)
        rc = self.lib.lmpc_ss_query_batch(self._h, C.c_int32(B), _ptr(q), _ptr(ss_x), _ptr(ss_j), _ptr(nf))
        self._check(rc, "lmpc_ss_query_batch")
        return ss_x, ss_j, nf

    # ---- fleet safe set: one recorder and one ring of laps per car, on the device (include/lmpc_hip.h) ----
    def fleet_ss_create(self, batch: int, max_pts_per_lap: int) -> int:
        """lmpc_fleet_ss_create: a store for `batch` cars, max_lap_stored laps of at most max_pts_per_lap samples each (replaces an
        earlier one).  Returns the bytes it allocated."""
        self.use_current_stream()
        self._check(self.lib.lmpc_fleet_ss_create(self._h, C.c_int32(int(batch)), C.c_int32(int(max_pts_per_lap))), "lmpc_fleet_ss_create")
        return self.fleet_ss_bytes()

    def fleet_ss_destroy(self):
        self._check(self.lib.lmpc_fleet_ss_destroy(self._h), "lmpc_fleet_ss_destroy")

    def fleet_ss_reset(self):
        """Empties every car's recorder and ring without reallocating."""
        self.use_current_stream()
        self._check(self.lib.lmpc_fleet_ss_reset(self._h), "lmpc_fleet_ss_reset")

    def fleet_ss_bytes(self) -> int:
        n = C.c_int64(0)
        self._check(self.lib.lmpc_fleet_ss_bytes(self._h, C.byref(n)), "lmpc_fleet_ss_bytes")
        return int(n.value)

    def fleet_ss_record(self, x, u, k, t: float, total_length: float, active=None):
        """lmpc_fleet_ss_record_batch: SafeSetRecorder.step for every car -- x [6][B], u [2][B], k [B] device tensors, t the time stamp;
        active (int32 [B], optional): 0 skips the car.  Asynchronous."""
        self.use_current_stream()
        x, u, k = self._t(x), self._t(u), self._t(k)
        if active is not None:
            active = self._torch.as_tensor(active, dtype=self._torch.int32, device=self.device).contiguous()
        rc = self.lib.lmpc_fleet_ss_record_batch(self._h, C.c_int32(x.shape[1]), _ptr(x), _ptr(u), _ptr(k), C.c_double(float(t)),
                                                 C.c_double(float(total_length)), _ptr(active))
        self._check(rc, "lmpc_fleet_ss_record_batch")

    def fleet_ss_query(self, query, out=None):
        """lmpc_fleet_ss_query_batch: ss_query with query b run against car b's own ring.  `out` = (ss_x [6][S][B], ss_j [S][B],
        n_found [B]) reuses the caller's buffers (the kernel writes every entry); otherwise they are allocated."""
        torch = self._torch
        self.use_current_stream()
        q = self._t(query)
        B = q.shape[1]
        S = int(self.config["num_ss_pts"])
        if out is not None:
            ss_x, ss_j, nf = out
        else:
            ss_x = torch.zeros((6, S, B), dtype=torch.float64, device=self.device)
            ss_j = torch.zeros((S, B), dtype=torch.float64, device=self.device)
            nf = torch.zeros((B,), dtype=torch.int32, device=self.device)
        rc = self.lib.lmpc_fleet_ss_query_batch(self._h, C.c_int32(B), _ptr(q), _ptr(ss_x), _ptr(ss_j), _ptr(nf))
        self._check(rc, "lmpc_fleet_ss_query_batch")
        return ss_x, ss_j, nf

    def fleet_ss_load(self, laps, total_length: float, car: int = -1):
        """lmpc_fleet_ss_load: laps = list of (x [n,6], u [n,2], k [n], t [n]) host arrays, oldest first, pushed into the ring of
        car `car` (-1: of every car)."""
        import numpy as np

        n_pts = np.array([np.asarray(l[0]).shape[0] for l in laps], dtype=np.int32)
        if len(laps):
            cat = [np.ascontiguousarray(np.concatenate([np.asarray(l[i], dtype=np.float64).reshape(n, -1) for l, n in zip(laps, n_pts)], 0))
                   for i in range(4)]
        else:
            cat = [np.zeros((0, w)) for w in (6, 2, 1, 1)]
        rc = self.lib.lmpc_fleet_ss_load(self._h, C.c_int32(int(car)), C.c_int32(len(laps)), n_pts.ctypes.data_as(C.c_void_p),
                                         *[a.ctypes.data_as(C.c_void_p) for a in cat], C.c_double(float(total_length)))
        self._check(rc, "lmpc_fleet_ss_load")

    def fleet_ss_get_laps(self, car: int):
        """lmpc_fleet_ss_get_laps: the closed laps of one car, oldest first, as a list of (x [n,6], u [n,2], k [n], t [n]) host arrays."""
        import numpy as np

        n_laps = C.c_int32(0)
        n_pts = np.zeros(max(int(self.config["max_lap_stored"]), 1), dtype=np.int32)
        rc = self.lib.lmpc_fleet_ss_get_laps(self._h, C.c_int32(int(car)), C.byref(n_laps), n_pts.ctypes.data_as(C.c_void_p), None, None, None, None)
        self._check(rc, "lmpc_fleet_ss_get_laps")
        n_pts = n_pts[:n_laps.value]
        n = int(n_pts.sum())
        x, u, k, t = np.zeros((n, 6)), np.zeros((n, 2)), np.zeros(n), np.zeros(n)
        if n:
            n_pts2 = np.zeros(max(int(self.config["max_lap_stored"]), 1), dtype=np.int32)
            rc = self.lib.lmpc_fleet_ss_get_laps(self._h, C.c_int32(int(car)), C.byref(n_laps), n_pts2.ctypes.data_as(C.c_void_p),
                                                 *[a.ctypes.data_as(C.c_void_p) for a in (x, u, k, t)])
            self._check(rc, "lmpc_fleet_ss_get_laps")
        cuts = np.cumsum(n_pts)[:-1]
        return [tuple(parts) for parts in zip(*(np.split(a, cuts) for a in (x, u, k, t)))] if len(n_pts) else []

    def fleet_ss_stats(self, B: int, out=None):
        """lmpc_fleet_ss_stats: {"laps_in_ring", "lap_count", "n_dropped"} int32 [B] and "last_lap_time" float64 [B], device tensors;
        `out` (such a dict) reuses buffers.  Asynchronous."""
        torch = self._torch
        self.use_current_stream()
        if out is None:
            out = {key: torch.zeros((B,), dtype=torch.int32, device=self.device) for key in ("laps_in_ring", "lap_count", "n_dropped")}
            out["last_lap_time"] = torch.zeros((B,), dtype=torch.float64, device=self.device)
        rc = self.lib.lmpc_fleet_ss_stats(self._h, C.c_int32(B), _ptr(out.get("laps_in_ring")), _ptr(out.get("lap_count")),
                                          _ptr(out.get("n_dropped")), _ptr(out.get("last_lap_time")))
        self._check(rc, "lmpc_fleet_ss_stats")
        return out

    def fleet_loop_state(self, B: int, n_rec: int):
        """The caller-owned device arrays of fleet_loop_advance for a fresh experiment, zero-filled: phase, n_learn [B], lap_kind
        [n_rec][B], counters [2] (int32), lap_time [n_rec][B], x_ic [6][B], query [2][B] (float64)."""
        torch = self._torch
        i32, f64 = dict(dtype=torch.int32, device=self.device), dict(dtype=torch.float64, device=self.device)
        return {"phase": torch.zeros(B, **i32), "n_learn": torch.zeros(B, **i32), "lap_kind": torch.zeros((n_rec, B), **i32),
                "counters": torch.zeros(2, **i32), "lap_time": torch.zeros((n_rec, B), **f64), "x_ic": torch.zeros((6, B), **f64),
                "query": torch.zeros((2, B), **f64)}

    def fleet_loop_advance(self, track: dict, inp: dict, sol_trk, sol_lrn, x, u_prev, state: dict, dt: float, dt_sim: float, n_sub: int = 1,
                           t: float = 0.0, speed_scale=(1.0, 1.0), speed_limit=(None, None), max_vel_ref_diff=(None, None),
                           restart_failed: bool = False, warm_laps: int = 2, learn_laps: int = 4, switch_phase: bool = True, plant=None,
                           distance=None, worst_excess=None, n_fail=None, n_rec: int | None = None, dtrack: bool = False, gamma_y=None):
        """lmpc_fleet_loop_advance_batch on this (the learning) solver, which owns the fleet store: everything between two solves of a
        fleet LMPC period in one launch -- per car the solution of the controller it drives with (state["phase"]: 0 `sol_trk`, 1
        `sol_lrn`; each a dict with X_optm, U_optm, status, or None when that controller did not run), input and plant, the next
        references in place in `inp`, state["x_ic"], the car's recorder and ring, the lap book (state["lap_time"], ["lap_kind"],
        ["n_learn"]), the phase and state["counters"], and state["query"].  Both solutions None: the head-only call of period 0.
        speed_scale / speed_limit / max_vel_ref_diff: (tracking, learning) pairs; a None limit is this solver's x_max[3], a None
        difference its max_vel_ref_diff.  plant: a vehicle dict for the plant (None: this solver's, or while a car table is set --
        set_car_vehicles -- car b's own vehicle; the library refuses plant= then).  `state` is fleet_loop_state's
        dict; n_rec (default: the lap book's first dimension) is how many of its rows the call may write.
        dtrack=True: lmpc_fleet_loop_advance_dtrack_batch (include/lmpc_hip_fleet_dtrack.h) -- the same call with car b's plant the
        four-wheel vehicle b of the double-track table (set_dtrack_vehicles; the library refuses plant= and a car table then);
        gamma_y (a float64 [B] tensor, optional, with dtrack=True only) receives plant_step_dtrack's gamma_y.  Asynchronous; nothing
        is read back."""
        self.use_current_stream()
        ct = self._ctrack(track)
        io = CFleetLoop()
        for pre, sol in (("trk", sol_trk), ("lrn", sol_lrn)):
            for name, key in (("X_", "X_optm"), ("U_", "U_optm"), ("status_", "status")):
                setattr(io, name + pre, _ptr(None if sol is None else sol.get(key)))
        io.x, io.u_prev = _ptr(x), _ptr(u_prev)
        for key in ("X_ref", "U_ref", "T_ref", "bound_left", "bound_right", "curvatures", "vel_ref"):
            setattr(io, key, _ptr(inp.get(key)))
        io.dt, io.dt_sim, io.t = float(dt), float(dt_sim), float(t)
        for i in range(2):
            io.speed_scale[i] = float(speed_scale[i])
            io.speed_limit[i] = float(self.config["x_max"][3] if speed_limit[i] is None else speed_limit[i])
            io.max_vel_ref_diff[i] = float(self.config["max_vel_ref_diff"] if max_vel_ref_diff[i] is None else max_vel_ref_diff[i])
        io.n_sub, io.restart_failed, io.warm_laps, io.learn_laps = int(n_sub), int(bool(restart_failed)), int(warm_laps), int(learn_laps)
        io.switch_phase = int(bool(switch_phase))
        lap_time = state.get("lap_time")
        io.n_rec = int(n_rec) if n_rec is not None else (int(lap_time.shape[0]) if lap_time is not None else 0)
        if lap_time is not None and io.n_rec > int(lap_time.shape[0]):
            raise ValueError("fleet_loop_advance: n_rec exceeds the lap book's rows")
        cv = None
        if plant is not None:
            cv = _fill(CVehicle(), plant)
            io.plant = C.pointer(cv)
        for key in ("phase", "n_learn", "lap_time", "lap_kind", "counters", "x_ic", "query"):
            setattr(io, key, _ptr(state.get(key)))
        io.distance, io.worst_excess, io.n_fail = _ptr(distance), _ptr(worst_excess), _ptr(n_fail)
        if dtrack:
            rc = self.lib.lmpc_fleet_loop_advance_dtrack_batch(self._h, C.c_int32(x.shape[1]), C.byref(ct), C.byref(io), _ptr(gamma_y))
            self._check(rc, "lmpc_fleet_loop_advance_dtrack_batch")
            return
        if gamma_y is not None:
            raise ValueError("fleet_loop_advance: gamma_y= goes with dtrack=True")
        rc = self.lib.lmpc_fleet_loop_advance_batch(self._h, C.c_int32(x.shape[1]), C.byref(ct), C.byref(io))
        self._check(rc, "lmpc_fleet_loop_advance_batch")

    # ---- per-car error-dynamics regression on the fleet safe set (safe_set.cpp:182-245, one SafeSetManager per car) ----
    def fleet_ss_set_regression(self, in_state=(3, 4, 5), in_ctrl=(0, 1), out_rows=(3, 4, 5), dist_max: float = 1.0,
                                as_written: bool = False, off: bool = False, rows=None):
        """lmpc_fleet_ss_set_regression: from now on every fp64 / mixed solve of this solver (and fleet_ss_regress) corrects problem
        b's model by the regression on car b's OWN closed laps in the fleet store, as they are at each call; nothing is uploaded.
        in_state, in_ctrl, out_rows: one feature list for all regressed rows;
        rows = {row: (in_state, in_ctrl), ...}: one list per regressed row instead (lmpc_fleet_ss_set_regression_rows), with
        the three one-list keywords left at their defaults.
        in_state=None or off=True switches it off.  as_written: the reference's literal signs (set_regression_laps)."""
        self.use_current_stream()
        _rows_exclude_one_list(rows, in_state, in_ctrl, out_rows)
        if off or in_state is None:
            self._check(self.lib.lmpc_fleet_ss_set_regression(self._h, None), "lmpc_fleet_ss_set_regression")
            return
        if rows is not None:
            spec = _rows_spec(rows, dist_max, as_written)
            self._check(self.lib.lmpc_fleet_ss_set_regression_rows(self._h, C.byref(spec)), "lmpc_fleet_ss_set_regression_rows")
            return
        spec = CRegressionSpec()
        spec.n_out, spec.n_in_state, spec.n_in_ctrl, spec.dist_max = len(out_rows), len(in_state), len(in_ctrl), float(dist_max)
        spec.out[:len(out_rows)] = list(out_rows)
        spec.in_state[:len(in_state)] = list(in_state)
        spec.in_ctrl[:len(in_ctrl)] = list(in_ctrl)
        spec.as_written = 1 if as_written else 0
        self._check(self.lib.lmpc_fleet_ss_set_regression(self._h, C.byref(spec)), "lmpc_fleet_ss_set_regression")

    def fleet_ss_regress(self, inp: dict, A, Bm, g):
        """lmpc_fleet_ss_regress_batch: regress() with problem b run against car b's own ring -- adds RegResult onto A [6,6,N-1,B],
        Bm [6,2,N-1,B], g [6,N-1,B] (device tensors, in place).  Asynchronous."""
        self.use_current_stream()
        X, U = self._t(inp["X_ref"]), self._t(inp["U_ref"])
        rc = self.lib.lmpc_fleet_ss_regress_batch(self._h, C.c_int32(X.shape[2]), _ptr(X), _ptr(U), _ptr(A), _ptr(Bm), _ptr(g))
        self._check(rc, "lmpc_fleet_ss_regress_batch")
        return A, Bm, g

    # ---- spline track: the interpolants on the device, global <-> Frenet (racing_trajectory.cpp:25-236; include/lmpc_hip.h) ----
    def spline_track(self, tr) -> SplineTrack:
        """lmpc_spline_track_create from a RacingTrajectory (or the dict its to_spline_track() returns): uploads once."""
        import numpy as np
        self.use_current_stream()
        d = tr if isinstance(tr, dict) else tr.to_spline_track()
        arr = {k: np.ascontiguousarray(d[k], dtype=np.float64) for k in ("breaks", "coef", "wp_x", "wp_y", "wp_s")}
        P, n_wp = arr["breaks"].size - 1, arr["wp_s"].size
        if arr["coef"].shape != (5, P, 4) or arr["wp_x"].size != n_wp or arr["wp_y"].size != n_wp:
            raise ValueError("spline_track: coef must be [5][P][4] for P + 1 breaks, and wp_x, wp_y, wp_s of one length")
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
        p = C.c_void_p(0)
        rc = self.lib.lmpc_spline_track_create(self._h, C.c_double(float(d["L"])), C.c_int32(P), dp(arr["breaks"]), dp(arr["coef"]),
                                               C.c_int32(n_wp), dp(arr["wp_x"]), dp(arr["wp_y"]), dp(arr["wp_s"]), C.byref(p))
        self._check(rc, "lmpc_spline_track_create")
        return SplineTrack(self, p, float(d["L"]), float(np.median(np.diff(arr["wp_s"]))), n_wp)

    def track_sample(self, track: SplineTrack, s, out=None):
        """lmpc_track_sample_batch: the interpolants at the abscissae s [n] (any value: wrapped) -> float64 [7][n] =
        x, y, yaw, curvature (as written upstream), left, right, vel."""
        self.use_current_stream()
        s = self._t(s).reshape(-1)
        if out is None:
            out = self._torch.empty((7, s.numel()), dtype=self._torch.float64, device=self.device)
        self._check(self.lib.lmpc_track_sample_batch(self._h, track._p, C.c_int32(s.numel()), _ptr(s), _ptr(out)), "lmpc_track_sample_batch")
        return out

    def tabulate_track(self, track: SplineTrack, M: int = 1024) -> dict:
        """lmpc_spline_track_tabulate: the uniform tables of an lmpc_track (what RacingTrajectory.to_track_table samples on the host),
        filled on the device; the returned dict goes wherever a `track` is expected."""
        torch = self._torch
        self.use_current_stream()
        out = {k: torch.empty((M,), dtype=torch.float64, device=self.device) for k in ("curvature", "bound_left", "bound_right", "vel")}
        rc = self.lib.lmpc_spline_track_tabulate(self._h, track._p, C.c_int32(M), *[_ptr(out[k]) for k in ("curvature", "bound_left", "bound_right", "vel")])
        self._check(rc, "lmpc_spline_track_tabulate")
        out["L"], out["M"] = track.L, int(M)
        return out

    def global_to_frenet(self, track: SplineTrack, pose, s0=None, seeded=None, out=None):
        """lmpc_global_to_frenet_batch: pose [3][B] = (x, y, yaw) -> (frenet [3][B] = (s, t, xi), status int32 [B]: TRACK_*).  s0 [B]
        starts the search of the poses with seeded[b] != 0 (int32 [B]; None: all of them), the others start at the nearest
        waypoint.  `out` = (frenet, status) reuses buffers.  Asynchronous."""
        torch = self._torch
        self.use_current_stream()
        pose = self._t(pose)
        B = pose.shape[1]
        if s0 is not None:
            s0 = self._t(s0)
        if seeded is not None:
            if s0 is None:
                raise ValueError("global_to_frenet: `seeded` needs s0")
            seeded = torch.as_tensor(seeded, dtype=torch.int32, device=self.device).contiguous()
        frenet, status = out if out is not None else (torch.empty((3, B), dtype=torch.float64, device=self.device),
                                                      torch.empty((B,), dtype=torch.int32, device=self.device))
        rc = self.lib.lmpc_global_to_frenet_batch(self._h, track._p, C.c_int32(B), _ptr(pose), _ptr(s0), _ptr(seeded), _ptr(frenet), _ptr(status))
        self._check(rc, "lmpc_global_to_frenet_batch")
        return frenet, status

    def frenet_to_global(self, track: SplineTrack, X, out=None):
        """lmpc_frenet_to_global_batch: rows 0 - 2 of X [6][n][B] (a plan) or [6][B] (car states; any leading size >= 3) ->
        pose [3][n][B] / [3][B] = (x, y, yaw).  Asynchronous."""
        torch = self._torch
        self.use_current_stream()
        X = self._t(X)
        if X.dim() not in (2, 3) or X.shape[0] < 3:
            raise ValueError("frenet_to_global: X is [>= 3][n][B] or [>= 3][B]")
        shape = (3,) + tuple(X.shape[1:])
        n, B = (1, X.shape[1]) if X.dim() == 2 else (X.shape[1], X.shape[2])
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=self.device)
        self._check(self.lib.lmpc_frenet_to_global_batch(self._h, track._p, C.c_int32(B), C.c_int32(n), _ptr(X), _ptr(out)), "lmpc_frenet_to_global_batch")
        return out

    # ---- batched extended Kalman filter, one per car (ekf_state_estimator.cpp:112-214; include/lmpc_hip.h) ----
    def ekf_create(self, batch: int, x0, P0, Q, x_min, x_max):
        """lmpc_ekf_create: `batch` filters over this solver's vehicle, every car started at x0 [6], P0 [6,6]; Q [6,6] is added per
        update, [x_min, x_max] clips the estimate.  Replaces an earlier filter."""
        import numpy as np

        self.use_current_stream()
        cfg = CEkfConfig()
        for name, v, n in (("x0", x0, 6), ("P0", P0, 36), ("Q", Q, 36), ("x_min", x_min, 6), ("x_max", x_max, 6)):
            a = np.asarray(v, dtype=np.float64).reshape(-1)
            if a.size != n:
                raise ValueError(f"ekf_create: {name} needs {n} values")
            getattr(cfg, name)[:] = [float(e) for e in a]
        self._check(self.lib.lmpc_ekf_create(self._h, C.c_int32(int(batch)), C.byref(cfg)), "lmpc_ekf_create")
        self._ekf_nz, self._ekf_B = [], int(batch)

    def ekf_destroy(self):
        self._check(self.lib.lmpc_ekf_destroy(self._h), "lmpc_ekf_destroy")

    def ekf_register_observation(self, rows) -> int:
        """lmpc_ekf_register_observation: an observation of the state rows `rows` (1 .. 6 distinct rows, in the order of z; a yaw row
        is aligned to its measurement).  Returns the id ekf_update takes.  Before ekf_initialize only."""
        self.use_current_stream()
        rows = [int(r) for r in rows]
        arr = (C.c_int32 * max(len(rows), 1))(*rows)
        oid = C.c_int32(-1)
        self._check(self.lib.lmpc_ekf_register_observation(self._h, C.c_int32(len(rows)), arr, C.byref(oid)), "lmpc_ekf_register_observation")
        self._ekf_nz.append(len(rows))
        return int(oid.value)

    def ekf_initialize(self, timestamp_ns: int):
        self._check(self.lib.lmpc_ekf_initialize(self._h, C.c_int64(int(timestamp_ns))), "lmpc_ekf_initialize")

    def ekf_set_state(self, x=None, P=None):
        """lmpc_ekf_set_state: per-car start, x [6][B] and P [36][B] or [6][6][B] device tensors; None broadcasts the config's x0 / P0."""
        self.use_current_stream()
        x = None if x is None else self._t(x)
        P = None if P is None else self._t(P)
        self._check(self.lib.lmpc_ekf_set_state(self._h, C.c_int32(self._ekf_B), _ptr(x), _ptr(P)), "lmpc_ekf_set_state")

    def ekf_update_control(self, u):
        """lmpc_ekf_update_control: u [2][B], held over the predictions until the next call.  Asynchronous."""
        self.use_current_stream()
        u = self._t(u)
        self._check(self.lib.lmpc_ekf_update_control(self._h, C.c_int32(u.shape[1]), _ptr(u)), "lmpc_ekf_update_control")

    def ekf_update(self, obs_id: int, z, R, timestamp_ns: int, out=None):
        """lmpc_ekf_update_batch: one update of every filter -- the prediction to timestamp_ns and, with obs_id >= 0, the correction by
        z [nz][B], R [nz][nz][B] (a car with a NaN or Inf in either takes the pure prediction); obs_id = -1 (z, R None): prediction
        only.  Returns (x [6][B], P [6][6][B], Kz [6][nz][B] or None, flags int32 [B]: EKF_*); `out` = such a tuple reuses the
        caller's buffers, and an entry None in it is not asked of the kernel.  Asynchronous."""
        torch = self._torch
        self.use_current_stream()
        B = self._ekf_B
        nz = self._ekf_nz[obs_id] if 0 <= obs_id < len(self._ekf_nz) else 0
        z = None if z is None else self._t(z)
        R = None if R is None else self._t(R)
        if out is not None:
            x, P, Kz, flags = out
        else:
            kw = dict(dtype=torch.float64, device=self.device)
            x, P = torch.empty((6, B), **kw), torch.empty((6, 6, B), **kw)
            Kz = torch.empty((6, nz, B), **kw) if nz else None
            flags = torch.empty((B,), dtype=torch.int32, device=self.device)
        rc = self.lib.lmpc_ekf_update_batch(self._h, C.c_int32(B if z is None else z.shape[-1]), C.c_int32(int(obs_id)), _ptr(z), _ptr(R),
                                            C.c_int64(int(timestamp_ns)), _ptr(x), _ptr(P), _ptr(Kz), _ptr(flags))
        self._check(rc, "lmpc_ekf_update_batch")
        return x, P, Kz, flags

    def ekf_get(self):
        """lmpc_ekf_get: {"x" [6][B], "P" [6][6][B], "K" [6][sum nz][B]} device tensors, "timestamp_ns", "initialized"."""
        torch = self._torch
        self.use_current_stream()
        B, nzs = self._ekf_B, sum(self._ekf_nz)
        kw = dict(dtype=torch.float64, device=self.device)
        x, P, K = torch.empty((6, B), **kw), torch.empty((6, 6, B), **kw), torch.zeros((6, nzs, B), **kw)
        ns, init = C.c_int64(0), C.c_int32(0)
        self._check(self.lib.lmpc_ekf_get(self._h, C.c_int32(B), _ptr(x), _ptr(P), _ptr(K), C.byref(ns), C.byref(init)), "lmpc_ekf_get")
        return {"x": x, "P": P, "K": K, "timestamp_ns": int(ns.value), "initialized": bool(init.value)}

    # ---- the fused estimated period (include/lmpc_hip_estimated.h) ----
    def loop_advance_estimated(self, track: dict, spline: SplineTrack, inp: dict, sol: dict, x, u_prev, x_ic, dt: float, dt_sim: float, n_sub: int,
                               obs_vel: int, obs_pose: int, t_vel_ns: int, t_pose_ns: int, noise_vel, R_vel, noise_pose, R_pose,
                               speed_scale: float = 1.0, speed_limit: float | None = None, restart_failed: bool = True, x_est=None, z_vel=None,
                               z_pose=None, ekf_flags=None, track_status=None, distance=None, worst_excess=None, n_fail=None, sq_err=None):
        """lmpc_loop_advance_estimated_batch: one period of the estimated closed loop behind a solve, in one launch -- the input applied
        (to u_prev and to the filter), the TRUTH x [6][B] stepped in two halves with the velocity observation (rows of obs_vel, plus
        noise_vel [nz_v][B]) between them and the pose observation (rows of obs_pose, plus noise_pose [nz_p][B]; a NaN drops the
        car's measurement) behind them, the two filter updates at t_vel_ns and t_pose_ns, the estimate projected into x_ic [6][B]
        (seeded with the incoming x_ic[0]), and the next references in `inp` (shift; for a failed car the old plan shifted in place
        or, restart_failed, a cold start at the new x_ic).  x, u_prev, x_ic and inp's seven arrays are updated in place.  Optional:
        x_est [6][B] (global estimate), z_vel, z_pose (the measurements formed), and the accumulators ekf_flags int32 [B] (|=),
        track_status int32 [B] (max), distance, worst_excess [B], n_fail int64 [B], sq_err [6][B].  The tensors are passed as they are
        (float64 / int32 / int64, contiguous, on the device).  Asynchronous; no torch operation, nothing read back."""
        self.use_current_stream()
        ct = self._ctrack(track)
        if speed_limit is None:
            speed_limit = float(self.config["x_max"][3])
        io = CEstimatedLoop()
        ptrs = dict(X_optm=sol["X_optm"], U_optm=sol["U_optm"], status=sol["status"], x=x, u_prev=u_prev, x_ic=x_ic, noise_vel=noise_vel, R_vel=R_vel,
                    noise_pose=noise_pose, R_pose=R_pose, x_est=x_est, z_vel=z_vel, z_pose=z_pose, ekf_flags=ekf_flags, track_status=track_status,
                    distance=distance, worst_excess=worst_excess, n_fail=n_fail, sq_err=sq_err,
                    **{k: inp[k] for k in ("X_ref", "U_ref", "T_ref", "bound_left", "bound_right", "curvatures", "vel_ref")})
        for name, t in ptrs.items():
            if t is not None and not t.is_contiguous():
                raise ValueError(f"loop_advance_estimated: {name} must be contiguous (it is passed by pointer)")
            setattr(io, name, None if t is None else t.data_ptr())
        io.dt, io.dt_sim, io.speed_scale, io.speed_limit = float(dt), float(dt_sim), float(speed_scale), float(speed_limit)
        io.n_sub, io.restart_failed, io.obs_vel, io.obs_pose = int(n_sub), 1 if restart_failed else 0, int(obs_vel), int(obs_pose)
        io.t_vel_ns, io.t_pose_ns = int(t_vel_ns), int(t_pose_ns)
        rc = self.lib.lmpc_loop_advance_estimated_batch(self._h, C.c_int32(x.shape[1]), C.byref(ct), spline._p, C.byref(io))
        self._check(rc, "lmpc_loop_advance_estimated_batch")

    # ---- batched time-varying LQR, one controller per car (racing_lqr.cpp:45-96; include/lmpc_hip.h) ----
    def lqr_create(self, cfg: dict, max_batch: int):
        """lmpc_lqr_create: controllers for up to `max_batch` cars over this solver's vehicle.  cfg: N (its own horizon, >= 2), dt,
        Q [6,6], R [2,2], Qf [6,6] -- general dense matrices, nothing is symmetrised (presets.sample_lqr).  Allocates the workspace
        and replaces an earlier controller."""
        import numpy as np

        self.use_current_stream()
        c = CLqrConfig()
        c.N, c.reserved, c.dt = int(cfg["N"]), 0, float(cfg["dt"])
        for name, n in (("Q", 36), ("R", 4), ("Qf", 36)):
            a = np.asarray(cfg[name], dtype=np.float64).reshape(-1)
            if a.size != n:
                raise ValueError(f"lqr_create: {name} needs {n} values")
            getattr(c, name)[:] = [float(e) for e in a]
        self._check(self.lib.lmpc_lqr_create(self._h, C.c_int32(int(max_batch)), C.byref(c)), "lmpc_lqr_create")
        self._lqr_N = int(cfg["N"])

    def lqr_destroy(self):
        self._check(self.lib.lmpc_lqr_destroy(self._h), "lmpc_lqr_destroy")
        self._lqr_N = None

    def lqr_solve(self, x_ic, X_ref, U_ref, out=None, gains=False):
        """lmpc_lqr_solve_batch: x_ic [6][B], X_ref [6][N][B], U_ref [2][N-1][B] -> {"X_optm" [6][N][B], "U_optm" [2][N-1][B],
        "u" [2][B] (a view of U_optm), "flags" int32 [B]: LQR_NOT_FINITE}, and with gains=True "K" [2][6][N-1][B] and "P0" [6][6][B].
        `out` = such a dict reuses the caller's buffers; its "K", "P0" and "flags" may be None or missing and are then not asked of
        the kernels.  Two launches, asynchronous."""
        torch = self._torch
        self.use_current_stream()
        x_ic, X_ref, U_ref = self._t(x_ic), self._t(X_ref), self._t(U_ref)
        N = getattr(self, "_lqr_N", None)
        B = x_ic.shape[-1]
        if N is not None and (tuple(x_ic.shape) != (6, B) or tuple(X_ref.shape) != (6, N, B) or tuple(U_ref.shape) != (2, N - 1, B)):
            raise ValueError(f"lqr_solve: x_ic [6][B], X_ref [6][{N}][B], U_ref [2][{N - 1}][B] with one B, got "
                             f"{tuple(x_ic.shape)}, {tuple(X_ref.shape)}, {tuple(U_ref.shape)}")
        if out is None:
            kw = dict(dtype=torch.float64, device=self.device)
            n = N if N is not None else X_ref.shape[1]
            out = {"X_optm": torch.empty((6, n, B), **kw), "U_optm": torch.empty((2, n - 1, B), **kw),
                   "flags": torch.empty((B,), dtype=torch.int32, device=self.device)}
            if gains:
                out["K"], out["P0"] = torch.empty((2, 6, n - 1, B), **kw), torch.empty((6, 6, B), **kw)
        rc = self.lib.lmpc_lqr_solve_batch(self._h, C.c_int32(B), _ptr(x_ic), _ptr(X_ref), _ptr(U_ref), _ptr(out["X_optm"]), _ptr(out["U_optm"]),
                                           _ptr(out.get("K")), _ptr(out.get("P0")), _ptr(out.get("flags")))
        self._check(rc, "lmpc_lqr_solve_batch")
        out["u"] = out["U_optm"][:, 0, :]
        return out

    # ---- batched vanilla controller, one per car: pure pursuit + PID (vanilla_controller.cpp:49-109; include/lmpc_hip.h) ----
    def vanilla_create(self, cfg: dict, batch: int):
        """lmpc_vanilla_create: one controller per car for `batch` cars over this solver's vehicle, PID state zeroed.  cfg: the fields
        of lmpc_vanilla_config (presets.vanilla_controller).  Replaces an earlier store."""
        self.use_current_stream()
        c = _fill(CVanillaConfig(), cfg)
        self._check(self.lib.lmpc_vanilla_create(self._h, C.c_int32(int(batch)), C.byref(c)), "lmpc_vanilla_create")
        self._vanilla_B = int(batch)

    def vanilla_destroy(self):
        self._check(self.lib.lmpc_vanilla_destroy(self._h), "lmpc_vanilla_destroy")
        self._vanilla_B = None

    def vanilla_reset(self, B: int, integral=None):
        """lmpc_vanilla_reset: error and last_error to zero, the integral to `integral` [B] (None: zero).  Asynchronous."""
        self.use_current_stream()
        if integral is not None:
            integral = self._t(integral)
            if tuple(integral.shape) != (int(B),):
                raise ValueError(f"vanilla_reset: integral is [{B}]")
        self._check(self.lib.lmpc_vanilla_reset(self._h, C.c_int32(int(B)), _ptr(integral)), "lmpc_vanilla_reset")

    def vanilla_get(self, B: int) -> dict:
        """lmpc_vanilla_get: {"integral", "error", "last_error"} float64 [B], device tensors.  Asynchronous."""
        torch = self._torch
        self.use_current_stream()
        out = torch.empty((3, int(B)), dtype=torch.float64, device=self.device)
        self._check(self.lib.lmpc_vanilla_get(self._h, C.c_int32(int(B)), _ptr(out[0]), _ptr(out[1]), _ptr(out[2])), "lmpc_vanilla_get")
        return {"integral": out[0], "error": out[1], "last_error": out[2]}

    def vanilla_solve(self, track: SplineTrack, x_ic, vel_ref=None, speed_scale: float = 1.0, out=None):
        """lmpc_vanilla_solve_batch: one control decision per car.  x_ic [6][B]; vel_ref [B], or None for the track's velocity
        interpolant at the car's abscissa times speed_scale -> {"u_out" [3][B] = (FD, FB, STEER) in newtons and radians, "u_model"
        [2][B] = (u_a force_to_lon, STEER), "flags" int32 [B]: VANILLA_NOT_FINITE}.  `out` = such a dict reuses the caller's buffers;
        its "u_model" and "flags" may be None or missing and are then not asked of the kernel.  One launch, asynchronous."""
        torch = self._torch
        self.use_current_stream()
        x_ic = self._t(x_ic)
        if x_ic.dim() != 2 or x_ic.shape[0] != 6:
            raise ValueError(f"vanilla_solve: x_ic is [6][B], got {tuple(x_ic.shape)}")
        B = x_ic.shape[1]
        if vel_ref is not None:
            vel_ref = self._t(vel_ref)
            if tuple(vel_ref.shape) != (B,):
                raise ValueError(f"vanilla_solve: vel_ref is [{B}], got {tuple(vel_ref.shape)}")
        if out is None:
            kw = dict(dtype=torch.float64, device=self.device)
            out = {"u_out": torch.empty((3, B), **kw), "u_model": torch.empty((2, B), **kw),
                   "flags": torch.empty((B,), dtype=torch.int32, device=self.device)}
        rc = self.lib.lmpc_vanilla_solve_batch(self._h, C.c_int32(B), track._p if track is not None else None, _ptr(x_ic), _ptr(vel_ref),
                                               C.c_double(float(speed_scale)), _ptr(out.get("u_out")), _ptr(out.get("u_model")), _ptr(out.get("flags")))
        self._check(rc, "lmpc_vanilla_solve_batch")
        return out

    def vanilla_rollout(self, track: SplineTrack, table: dict, x, periods: int, dt_sim: float, n_sub: int = 1, speed_scale: float = 1.0,
                        logs: bool = True, distance=None, worst_excess=None, out=None):
        """lmpc_vanilla_rollout_batch: `periods` control periods of controller + plant per car in ONE launch.  x [6][B] is updated in
        place, as is the PID state; table: the track's uniform tables (device_track / tabulate_track); dt_sim, n_sub: the plant's
        sub-steps per period.  Returns {"X_log" [6][periods][B] the state each decision was taken at, "U_log" [2][periods][B] the
        u_model applied, "k_log" [periods][B] the table's curvature there (None with logs=False), "flags" int32 [B]}; distance and
        worst_excess (float64 [B], optional) are accumulated as loop_advance accumulates them.  `out` = such a dict reuses buffers; a
        None or missing entry is not asked of the kernel.  A flagged car is frozen at its last finite state and its logs are NaN
        from that period on.  Asynchronous."""
        torch = self._torch
        self.use_current_stream()
        if x.dim() != 2 or x.shape[0] != 6 or x.dtype != torch.float64 or not x.is_contiguous():
            raise ValueError("vanilla_rollout: x is a contiguous float64 [6][B] device tensor (it is updated in place)")
        B, P = x.shape[1], int(periods)
        ct = self._ctrack(table)
        if out is None:
            kw = dict(dtype=torch.float64, device=self.device)
            out = {"flags": torch.empty((B,), dtype=torch.int32, device=self.device)}
            if logs and P >= 1:
                out.update(X_log=torch.empty((6, P, B), **kw), U_log=torch.empty((2, P, B), **kw), k_log=torch.empty((P, B), **kw))
        rc = self.lib.lmpc_vanilla_rollout_batch(self._h, C.c_int32(B), track._p if track is not None else None, C.byref(ct), _ptr(x), C.c_int32(P),
                                                 C.c_double(float(dt_sim)), C.c_int32(int(n_sub)), C.c_double(float(speed_scale)),
                                                 _ptr(out.get("X_log")), _ptr(out.get("U_log")), _ptr(out.get("k_log")), _ptr(distance),
                                                 _ptr(worst_excess), _ptr(out.get("flags")))
        self._check(rc, "lmpc_vanilla_rollout_batch")
        return out

    def vanilla_rollout_fleet(self, track: SplineTrack, table: dict, x, periods: int, dt_sim: float, n_sub: int = 1, *, plant: str = "handle",
                              record=None, period0: int = 0, dt=None, u_prev=None, speed_scale: float = 1.0, logs: bool = False,
                              distance=None, worst_excess=None, out=None):
        """lmpc_vanilla_rollout_fleet_batch: vanilla_rollout with a plant per car and the fleet safe set's recorder inside the period
        loop, ONE launch for `periods` control periods.  plant: "handle" (this solver's vehicle: vanilla_rollout's plant, bit for bit),
        "cars" (car b on vehicle b of set_car_vehicles' table) or "dtrack" (car b on four-wheel vehicle b of set_dtrack_vehicles'
        table); the decision reads this solver's vehicle whatever the plant.  record: None, "applied" (sample p = the state of period
        p and the input applied from it, run_vanilla's convention) or "arrived" (the input that led to it, what fleet_loop_advance
        records; period 0 takes u_prev); the samples of live periods go to the fleet store (fleet_ss_create) with the time stamp
        (period0 + p) * dt.  u_prev (float64 [2][B], updated in place where given): on return the last input applied.  x [6][B] is
        updated in place, as is the PID state.  Returns vanilla_rollout's dictionary ("X_log", "U_log", "k_log" only with logs=True);
        `out` reuses buffers, a None or missing entry is not asked of the kernel.  Asynchronous."""
        torch = self._torch
        self.use_current_stream()
        if x.dim() != 2 or x.shape[0] != 6 or x.dtype != torch.float64 or not x.is_contiguous():
            raise ValueError("vanilla_rollout_fleet: x is a contiguous float64 [6][B] device tensor (it is updated in place)")
        B, P = x.shape[1], int(periods)
        if u_prev is not None and (tuple(u_prev.shape) != (2, B) or u_prev.dtype != torch.float64 or not u_prev.is_contiguous()):
            raise ValueError("vanilla_rollout_fleet: u_prev is a contiguous float64 [2][B] device tensor (it is updated in place)")
        if plant not in VANILLA_PLANT or record not in VANILLA_RECORD:
            raise ValueError("vanilla_rollout_fleet: plant is one of %s, record one of %s" % (sorted(VANILLA_PLANT), list(VANILLA_RECORD)))
        ct = self._ctrack(table)
        if out is None:
            kw = dict(dtype=torch.float64, device=self.device)
            out = {"flags": torch.empty((B,), dtype=torch.int32, device=self.device)}
            if logs and P >= 1:
                out.update(X_log=torch.empty((6, P, B), **kw), U_log=torch.empty((2, P, B), **kw), k_log=torch.empty((P, B), **kw))
        io = CVanillaFleetRollout()
        io.x, io.u_prev = _ptr(x), _ptr(u_prev)
        io.periods, io.n_sub, io.plant, io.record = P, int(n_sub), VANILLA_PLANT[plant], VANILLA_RECORD[record]
        io.dt_sim, io.speed_scale, io.period0, io.dt = float(dt_sim), float(speed_scale), int(period0), 0.0 if dt is None else float(dt)
        io.X_log, io.U_log, io.k_log = _ptr(out.get("X_log")), _ptr(out.get("U_log")), _ptr(out.get("k_log"))
        io.distance, io.worst_excess, io.flags = _ptr(distance), _ptr(worst_excess), _ptr(out.get("flags"))
        rc = self.lib.lmpc_vanilla_rollout_fleet_batch(self._h, C.c_int32(B), track._p if track is not None else None, C.byref(ct), C.byref(io))
        self._check(rc, "lmpc_vanilla_rollout_fleet_batch")
        return out
