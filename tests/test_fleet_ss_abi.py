"""The fleet safe set's surface, checked without a GPU: the library exports every lmpc_fleet_ss_* entry point, the header declares
them (test_abi.py then holds the header to pedantic C11 and to the exported symbols), and Solver mirrors them."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]

ENTRY_POINTS = ("lmpc_fleet_ss_create", "lmpc_fleet_ss_destroy", "lmpc_fleet_ss_reset", "lmpc_fleet_ss_bytes",
                "lmpc_fleet_ss_record_batch", "lmpc_fleet_ss_query_batch", "lmpc_fleet_ss_load", "lmpc_fleet_ss_get_laps",
                "lmpc_fleet_ss_stats")
METHODS = ("fleet_ss_create", "fleet_ss_record", "fleet_ss_query", "fleet_ss_load", "fleet_ss_get_laps", "fleet_ss_stats",
           "fleet_ss_reset", "fleet_ss_destroy", "fleet_ss_bytes")


def test_fleet_entry_points_are_exported_and_declared(pkg):
    lib = pkg.load_library()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "lmpc_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(lmpc_[a-z_0-9]+)\s*\(", text))
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in declared, name


def test_solver_mirrors_the_fleet_entry_points(pkg):
    for name in METHODS:
        assert callable(getattr(pkg.Solver, name, None)), name
    assert callable(getattr(pkg.closed_loop, "run_lmpc_fleet", None))


def test_null_handle_is_an_argument_error(pkg):
    """The entry points follow the file's convention for a null handle (no GPU is touched)."""
    import ctypes as C

    lib = pkg.load_library()
    assert lib.lmpc_fleet_ss_create(None, C.c_int32(4), C.c_int32(16)) == -1
    assert lib.lmpc_fleet_ss_reset(None) == -1
    assert lib.lmpc_fleet_ss_query_batch(None, C.c_int32(4), None, None, None, None) == -1
    assert lib.lmpc_fleet_ss_stats(None, C.c_int32(4), None, None, None, None) == -1
