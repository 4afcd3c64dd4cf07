"""The batched extended Kalman filter's surface, checked without a GPU: the library exports the eight lmpc_ekf_* entry points and the
header declares them (test_abi.py then holds the header to pedantic C11 and to the exported symbols), a null handle is an argument
error, Solver mirrors them, closed_loop has run_estimated, and the facade library holds the C++ class."""
import ctypes as C
import inspect
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "racing-lmpc-ros2_amd" / "lib"

ENTRY_POINTS = ("lmpc_ekf_create", "lmpc_ekf_destroy", "lmpc_ekf_register_observation", "lmpc_ekf_initialize", "lmpc_ekf_set_state",
                "lmpc_ekf_update_control", "lmpc_ekf_update_batch", "lmpc_ekf_get")
METHODS = ("ekf_create", "ekf_register_observation", "ekf_initialize", "ekf_set_state", "ekf_update_control", "ekf_update", "ekf_get")


def test_ekf_entry_points_are_exported_and_declared(pkg):
    lib = pkg.load_library()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "lmpc_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(lmpc_[a-z_0-9]+)\s*\(", text))
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in declared, name
    assert "lmpc_ekf_config" in text


def test_config_struct_matches_the_header(pkg):
    from importlib import import_module
    capi = import_module(pkg.__name__ + ".capi")
    assert C.sizeof(capi.CEkfConfig) == (6 + 36 + 36 + 6 + 6) * 8
    assert (pkg.EKF_FALLBACK, pkg.EKF_R_REPAIRED, pkg.EKF_NOT_FINITE) == (1, 2, 4)


def test_null_handle_is_an_argument_error(pkg):
    """Every entry point follows the file's convention for a null handle (no GPU is touched)."""
    lib = pkg.load_library()
    i32, i64 = C.c_int32, C.c_int64
    assert lib.lmpc_ekf_create(None, i32(4), None) == -1
    assert lib.lmpc_ekf_destroy(None) == -1
    assert lib.lmpc_ekf_register_observation(None, i32(2), None, None) == -1
    assert lib.lmpc_ekf_initialize(None, i64(0)) == -1
    assert lib.lmpc_ekf_set_state(None, i32(4), None, None) == -1
    assert lib.lmpc_ekf_update_control(None, i32(4), None) == -1
    assert lib.lmpc_ekf_update_batch(None, i32(4), i32(-1), None, None, i64(0), None, None, None, None) == -1
    assert lib.lmpc_ekf_get(None, i32(4), None, None, None, None, None) == -1


def test_solver_and_closed_loop_mirror_them(pkg):
    for name in METHODS:
        assert callable(getattr(pkg.Solver, name, None)), name
    assert inspect.signature(pkg.Solver.ekf_update).parameters["out"].default is None
    loop = inspect.signature(pkg.closed_loop.run_estimated)
    assert list(loop.parameters)[:6] == ["solver", "track", "spline", "x0", "u0", "steps"]
    assert loop.parameters["sensors"].default is None and loop.parameters["record_trace"].default is False and "seed" in loop.parameters


def test_facade_library_holds_the_cpp_class():
    """The class's methods are in liblmpc_racing_mpc.so's symbol table (by their Itanium-mangled names) and its driver is built."""
    so = LIB / "liblmpc_racing_mpc.so"
    assert so.exists() and (LIB / "test_ekf").exists(), "run __graft_entry__.build() first"
    blob = so.read_bytes()
    cls = "_ZN4lmpc15state_estimator19ekf_state_estimator17EKFStateEstimator"
    for method in ("register_observation", "initialize", "update_observation", "update_control"):
        assert f"{cls}{len(method)}{method}E".encode() in blob, method
    assert (cls + "C1E").encode() in blob or (cls + "C2E").encode() in blob
    for getter in ("get_latest_timestamp", "get_latest_estimate", "get_latest_estimate_covariance", "get_latest_kalman_gain", "is_initialized"):
        assert f"_ZNK4lmpc15state_estimator19ekf_state_estimator17EKFStateEstimator{len(getter)}{getter}Ev".encode() in blob, getter
