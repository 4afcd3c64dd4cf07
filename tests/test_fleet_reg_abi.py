"""The per-car regression's surface, checked without a GPU: the library exports lmpc_fleet_ss_set_regression and
lmpc_fleet_ss_regress_batch, the header declares them (test_abi.py then holds the header to pedantic C11 and to the exported symbols),
Solver mirrors them and run_lmpc_fleet takes the two arguments that use them."""
import inspect
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]

ENTRY_POINTS = ("lmpc_fleet_ss_set_regression", "lmpc_fleet_ss_regress_batch")
METHODS = ("fleet_ss_set_regression", "fleet_ss_regress")


def test_fleet_regression_entry_points_are_exported_and_declared(pkg):
    lib = pkg.load_library()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "lmpc_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(lmpc_[a-z_0-9]+)\s*\(", text))
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in declared, name


def test_solver_and_closed_loop_mirror_them(pkg):
    for name in METHODS:
        assert callable(getattr(pkg.Solver, name, None)), name
    sig = inspect.signature(pkg.Solver.fleet_ss_set_regression)
    for arg, default in (("in_state", (3, 4, 5)), ("in_ctrl", (0, 1)), ("out_rows", (3, 4, 5)), ("dist_max", 1.0), ("as_written", False),
                         ("off", False)):
        assert sig.parameters[arg].default == default, arg
    loop = inspect.signature(pkg.closed_loop.run_lmpc_fleet)
    assert loop.parameters["regression"].default is None and loop.parameters["plant"].default is None


def test_null_handle_is_an_argument_error(pkg):
    """Both entry points follow the file's convention for a null handle (no GPU is touched)."""
    import ctypes as C

    lib = pkg.load_library()
    assert lib.lmpc_fleet_ss_set_regression(None, None) == -1
    assert lib.lmpc_fleet_ss_regress_batch(None, C.c_int32(4), None, None, None, None, None) == -1
