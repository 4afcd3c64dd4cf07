"""lmpc_loop_advance_estimated_batch's surface, checked without a GPU: the library exports it, include/lmpc_hip_estimated.h declares it
and its struct and include/lmpc_hip.h itself does not (test_abi.py then holds the headers to pedantic C11 and to the exported
symbols), the ctypes mirror of the struct has the layout the C compiler gives it, a NULL handle is an argument error, and Solver /
closed_loop carry the methods with the signatures the loop's callers rely on."""
import ctypes as C
import inspect
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
NAME = "lmpc_loop_advance_estimated_batch"
MEMBERS = ("X_optm", "U_optm", "status", "x", "u_prev", "x_ic", "X_ref", "U_ref", "T_ref", "bound_left", "bound_right", "curvatures", "vel_ref",
           "dt", "dt_sim", "speed_scale", "speed_limit", "n_sub", "restart_failed", "obs_vel", "obs_pose", "t_vel_ns", "t_pose_ns",
           "noise_vel", "R_vel", "noise_pose", "R_pose", "x_est", "z_vel", "z_pose", "ekf_flags", "track_status", "distance", "worst_excess",
           "n_fail", "sq_err")


def _code(path):
    return re.sub(r"/\*.*?\*/", "", path.read_text(), flags=re.S)


def test_entry_point_is_exported_and_declared_in_the_new_header_only(pkg):
    lib = pkg.load_library()
    assert hasattr(lib, NAME)
    mine = _code(ROOT / "include" / "lmpc_hip_estimated.h")
    assert set(re.findall(r"\b(lmpc_[a-z_0-9]+)\s*\(", mine)) == {NAME}
    assert re.search(r"typedef\s+struct\s+lmpc_estimated_loop\s*\{", mine)
    for other in sorted((ROOT / "include").glob("*.h")):
        if other.name != "lmpc_hip_estimated.h":
            assert NAME not in _code(other) and "lmpc_estimated_loop" not in _code(other), other.name
    main = (ROOT / "include" / "lmpc_hip.h").read_text()
    at = main.index('#include "lmpc_hip_estimated.h"')
    assert main.index('extern "C" {') < main.index('#include "lmpc_hip_cars_model.h"') < at < main.rindex("#ifdef __cplusplus")
    assert pkg.capi._ABI_SYMBOLS_ESTIMATED == (NAME,)
    assert NAME not in pkg.capi._ABI_SYMBOLS


def test_the_unit_is_built_and_listed():
    """The eleventh translation unit, the new header among the Makefile's prerequisites, and the texts the kernel is made of: it
    includes the shared steps and defines no filter, projection or rollout of its own."""
    mk = (ROOT / "racing-lmpc-ros2_amd" / "csrc" / "Makefile").read_text()
    units = re.search(r"^UNITS := (.*)$", mk, flags=re.M).group(1).split() + [u for line in re.findall(r"^UNITS \+= (.*)$", mk, flags=re.M)
                                                                              for u in line.split()]
    assert units[10] == "lmpc_estimated_loop_kernel" and len(units) == len(set(units)) == 11
    assert (ROOT / "racing-lmpc-ros2_amd" / "csrc" / "lmpc_estimated_loop_kernel.hip").exists()
    assert "include/lmpc_hip_estimated.h" in re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1)
    csrc = ROOT / "racing-lmpc-ros2_amd" / "csrc"
    src = (csrc / "lmpc_estimated_loop_kernel.hip").read_text()
    for inc in ("lmpc_ekf_steps.hip.h", "lmpc_estimated.h", "lmpc_loop_steps.hip.h"):
        assert '#include "%s"' % inc in src, inc
    for text in ("LMPC_PLANT_SUBSTEPS(", "LMPC_CAR_COLD_RESTART(", "LMPC_CAR_SHIFT_IN_PLACE(", "lmpc_car_shift_knot(", "lmpc_ekf_predict_car(",
                 "lmpc_ekf_correct_car<", "track_project(", "track_to_global("):
        assert text in src, text
    assert not re.search(r"__shared__|__syncthreads|__shfl|atomic|lmpc_jvp|track_eval", src)
    # the stand-alone kernels are wrappers over the same functions
    ekf, trk = (csrc / "lmpc_ekf_kernel.hip").read_text(), (csrc / "lmpc_track_kernel.hip").read_text()
    assert "lmpc_ekf_predict_car(" in ekf and "lmpc_ekf_correct_car<NZ>(" in ekf and "lmpc_jvp" not in ekf
    assert "track_project(" in trk and "track_to_global(" in trk


def test_ctypes_mirror_has_the_c_layout(pkg, tmp_path):
    """The struct crosses the ABI by pointer: the mirror's size and the offset of every member must be the C compiler's, and the
    mirror's members are the header's, in its order."""
    CE = pkg.capi.CEstimatedLoop
    assert tuple(n for n, _ in CE._fields_) == MEMBERS
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "lmpc_hip.h"\nint main(void) {\n  printf("%zu\\n", sizeof(lmpc_estimated_loop));\n'
                   + "".join('  printf("%%zu\\n", offsetof(lmpc_estimated_loop, %s));\n' % m for m in MEMBERS) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", str(ROOT / "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(CE)] + [getattr(CE, m).offset for m in MEMBERS]


def test_null_handle_is_an_argument_error(pkg):
    lib = pkg.load_library()
    io = pkg.capi.CEstimatedLoop()
    assert lib.lmpc_loop_advance_estimated_batch(None, C.c_int32(4), None, None, C.byref(io)) == -1
    assert lib.lmpc_loop_advance_estimated_batch(None, C.c_int32(4), None, None, None) == -1


def test_solver_and_closed_loop_mirror_it(pkg):
    assert callable(getattr(pkg.Solver, "loop_advance_estimated", None))
    adv = inspect.signature(pkg.Solver.loop_advance_estimated).parameters
    for name in ("x_est", "z_vel", "z_pose", "ekf_flags", "track_status", "distance", "worst_excess", "n_fail", "sq_err"):
        assert adv[name].default is None, name
    plain = inspect.signature(pkg.closed_loop.run_estimated).parameters
    fused = inspect.signature(pkg.closed_loop.run_estimated_fused).parameters
    # run_estimated's arguments, name for name and default for default, then `poll`
    assert list(fused) == list(plain) + ["poll"]
    for name, p in plain.items():
        assert fused[name].default == p.default and fused[name].kind == p.kind, name
    assert fused["poll"].default == 0
