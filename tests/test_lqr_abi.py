"""The batched LQR's surface, checked without a GPU: the library exports the three lmpc_lqr_* entry points and the header declares
them (test_abi.py then holds the header to pedantic C11 and to the exported symbols), a null handle is an argument error, Solver
mirrors them, presets has sample_lqr, closed_loop has run_lqr, and the facade library holds the C++ class."""
import ctypes as C
import inspect
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "racing-lmpc-ros2_amd" / "lib"

ENTRY_POINTS = ("lmpc_lqr_create", "lmpc_lqr_destroy", "lmpc_lqr_solve_batch")


def test_lqr_entry_points_are_exported_and_declared(pkg):
    lib = pkg.load_library()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "lmpc_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(lmpc_[a-z_0-9]+)\s*\(", text))
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in declared, name
    assert "lmpc_lqr_config" in text and re.search(r"#define\s+LMPC_LQR_FLAG_NOT_FINITE\s+1\b", text)


def test_config_struct_matches_the_header(pkg):
    assert C.sizeof(pkg.CLqrConfig) == 8 + 8 + (36 + 4 + 36) * 8
    assert [f[0] for f in pkg.CLqrConfig._fields_] == ["N", "reserved", "dt", "Q", "R", "Qf"]
    assert pkg.LQR_NOT_FINITE == 1


def test_null_handle_is_an_argument_error(pkg):
    """Every entry point follows the file's convention for a null handle (no GPU is touched)."""
    lib = pkg.load_library()
    cfg = pkg.CLqrConfig()
    cfg.N, cfg.dt = 20, 0.01
    assert lib.lmpc_lqr_create(None, C.c_int32(4), C.byref(cfg)) == -1
    assert lib.lmpc_lqr_create(None, C.c_int32(4), None) == -1
    assert lib.lmpc_lqr_destroy(None) == -1
    assert lib.lmpc_lqr_solve_batch(None, C.c_int32(4), None, None, None, None, None, None, None, None) == -1


def test_solver_presets_and_closed_loop_mirror_them(pkg):
    assert list(inspect.signature(pkg.Solver.lqr_create).parameters) == ["self", "cfg", "max_batch"]
    assert list(inspect.signature(pkg.Solver.lqr_destroy).parameters) == ["self"]
    sig = inspect.signature(pkg.Solver.lqr_solve)
    assert list(sig.parameters) == ["self", "x_ic", "X_ref", "U_ref", "out", "gains"]
    assert sig.parameters["out"].default is None and sig.parameters["gains"].default is False
    assert list(inspect.signature(pkg.closed_loop.run_lqr).parameters) == ["solver", "x0", "X_traj", "U_traj", "steps"]
    sig = inspect.signature(pkg.presets.sample_lqr)
    assert sig.parameters["N"].default == 20 and sig.parameters["dt"].default == 0.01
    cfg = pkg.presets.sample_lqr()
    eye = lambda d: [[d[i] if i == j else 0.0 for j in range(len(d))] for i in range(len(d))]  # noqa: E731
    assert cfg == dict(N=20, dt=0.01, Q=eye([1.0] * 6), R=eye([1.0] * 2), Qf=eye([10.0, 10.0, 10.0, 1.0, 1.0, 10.0]))


def test_facade_library_holds_the_cpp_class():
    """The class's methods are in liblmpc_racing_mpc.so's symbol table (by their Itanium-mangled names) and its driver is built."""
    so = LIB / "liblmpc_racing_mpc.so"
    assert so.exists() and (LIB / "test_racing_lqr").exists(), "run __graft_entry__.build() first"
    blob = so.read_bytes()
    cls = "4lmpc3mpc10racing_lqr9RacingLQR"
    assert f"_ZN{cls}5solveE".encode() in blob
    assert f"_ZN{cls}9get_modelEv".encode() in blob
    assert f"_ZNK{cls}10get_configEv".encode() in blob
    assert f"_ZN{cls}C1E".encode() in blob or f"_ZN{cls}C2E".encode() in blob
