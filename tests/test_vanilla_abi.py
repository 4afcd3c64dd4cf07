"""The batched vanilla controller's surface, checked without a GPU: the library exports the six lmpc_vanilla_* entry points and the
header declares them and lmpc_vanilla_config (test_abi.py then holds the header to pedantic C11 and to the exported symbols), the
header compiles as C11 with the struct at the size the Python mirror has, a null handle is an argument error, Solver, presets,
ros_params and closed_loop mirror them, and the facade library holds the C++ class."""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "racing-lmpc-ros2_amd" / "lib"

# the seven exported names: six functions and the config struct they share
ENTRY_POINTS = ("lmpc_vanilla_create", "lmpc_vanilla_destroy", "lmpc_vanilla_reset", "lmpc_vanilla_get", "lmpc_vanilla_solve_batch",
                "lmpc_vanilla_rollout_batch")
FIELDS = ["lookahead_speed_ratio", "min_lookahead_distance", "max_lookahead_distance", "k_p", "k_i", "k_d", "min_cmd", "max_cmd", "min_i",
          "max_i", "dt", "force_to_lon"]


def test_vanilla_entry_points_are_exported_and_declared(pkg):
    lib = pkg.load_library()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "lmpc_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(lmpc_[a-z_0-9]+)\s*\(", text))
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in declared, name
    assert re.search(r"\}\s*lmpc_vanilla_config\s*;", text) and re.search(r"#define\s+LMPC_VANILLA_FLAG_NOT_FINITE\s+1\b", text)


def test_config_struct_matches_the_header(pkg, tmp_path):
    assert C.sizeof(pkg.CVanillaConfig) == 12 * 8
    assert [f[0] for f in pkg.CVanillaConfig._fields_] == FIELDS
    assert pkg.VANILLA_NOT_FINITE == 1
    # the header as C11: sizeof and the offset of the last field, checked by the compiler
    src = tmp_path / "vanilla_abi.c"
    src.write_text('#include <stddef.h>\n#include "lmpc_hip.h"\n'
                   "_Static_assert(sizeof(lmpc_vanilla_config) == 96, \"size\");\n"
                   "_Static_assert(offsetof(lmpc_vanilla_config, force_to_lon) == 88, \"last field\");\n"
                   "_Static_assert(offsetof(lmpc_vanilla_config, k_p) == 24, \"k_p\");\n"
                   "int (*p_solve)(lmpc_handle*, int32_t, const lmpc_spline_track*, const double*, const double*, double, double*, double*, int32_t*)"
                   " = lmpc_vanilla_solve_batch;\n"
                   "int (*p_roll)(lmpc_handle*, int32_t, const lmpc_spline_track*, const lmpc_track*, double*, int32_t, double, int32_t, double, double*,"
                   " double*, double*, double*, double*, int32_t*) = lmpc_vanilla_rollout_batch;\n")
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-c", str(src), "-o", str(tmp_path / "v.o")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


def test_null_handle_is_an_argument_error(pkg):
    """Every entry point follows the file's convention for a null handle (no GPU is touched)."""
    lib = pkg.load_library()
    cfg = pkg.CVanillaConfig()
    assert lib.lmpc_vanilla_create(None, C.c_int32(4), C.byref(cfg)) == -1
    assert lib.lmpc_vanilla_create(None, C.c_int32(4), None) == -1
    assert lib.lmpc_vanilla_destroy(None) == -1
    assert lib.lmpc_vanilla_reset(None, C.c_int32(4), None) == -1
    assert lib.lmpc_vanilla_get(None, C.c_int32(4), None, None, None) == -1
    assert lib.lmpc_vanilla_solve_batch(None, C.c_int32(4), None, None, None, C.c_double(1.0), None, None, None) == -1
    assert lib.lmpc_vanilla_rollout_batch(None, C.c_int32(4), None, None, None, C.c_int32(1), C.c_double(0.01), C.c_int32(1), C.c_double(1.0),
                                          None, None, None, None, None, None) == -1


def test_solver_presets_and_closed_loop_mirror_them(pkg):
    params = lambda f: list(inspect.signature(f).parameters)   # noqa: E731
    assert params(pkg.Solver.vanilla_create) == ["self", "cfg", "batch"]
    assert params(pkg.Solver.vanilla_reset) == ["self", "B", "integral"]
    assert params(pkg.Solver.vanilla_get) == ["self", "B"]
    assert params(pkg.Solver.vanilla_solve) == ["self", "track", "x_ic", "vel_ref", "speed_scale", "out"]
    assert params(pkg.Solver.vanilla_rollout)[:7] == ["self", "track", "table", "x", "periods", "dt_sim", "n_sub"]
    sig = inspect.signature(pkg.closed_loop.run_vanilla)
    assert list(sig.parameters) == ["solver", "track", "spline", "x0", "steps", "dt", "n_sub", "speed_scale", "chunk", "fused", "fleet_record"]
    assert sig.parameters["chunk"].default == 64 and sig.parameters["fused"].default is True and sig.parameters["fleet_record"].default is False
    for preset in (pkg.presets.vanilla_controller(), pkg.presets.vanilla_controller_2()):
        assert sorted(preset) == sorted(FIELDS) and preset["force_to_lon"] == 1e-3 and preset["dt"] == 0.1
    assert pkg.presets.vanilla_controller_2()["k_d"] == 0.1 and pkg.presets.vanilla_controller(1.0)["force_to_lon"] == 1.0
    assert "vanilla_config_from_params" in pkg.ros_params.__all__


def test_facade_library_holds_the_cpp_class():
    """The class's methods are in liblmpc_racing_mpc.so's symbol table (by their Itanium-mangled names) and its driver is built."""
    so = LIB / "liblmpc_racing_mpc.so"
    assert so.exists() and (LIB / "test_vanilla_controller").exists(), "run __graft_entry__.build() first"
    blob = so.read_bytes()
    cls = "4lmpc3mpc18vanilla_controller17VanillaController"
    assert f"_ZN{cls}5solveE".encode() in blob
    assert f"_ZN{cls}9get_modelEv".encode() in blob
    assert f"_ZNK{cls}10get_configEv".encode() in blob
    assert f"_ZN{cls}C1E".encode() in blob or f"_ZN{cls}C2E".encode() in blob
