"""lmpc_fleet_loop_advance_batch's surface, checked without a GPU: the library exports it, the header declares it and its struct
(test_abi.py then holds the header to pedantic C11 and to the exported symbols), the ctypes mirror of the struct has the size the
C compiler gives it, and Solver / closed_loop carry the methods."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_entry_point_is_exported_and_declared(pkg):
    lib = pkg.load_library()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "lmpc_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(lmpc_[a-z_0-9]+)\s*\(", text))
    assert hasattr(lib, "lmpc_fleet_loop_advance_batch")
    assert "lmpc_fleet_loop_advance_batch" in declared
    assert re.search(r"typedef\s+struct\s+lmpc_fleet_loop\s*\{", text)
    assert "lmpc_fleet_loop_advance_batch" in pkg.capi._ABI_SYMBOLS


def test_solver_and_closed_loop_mirror_it(pkg):
    assert callable(getattr(pkg.Solver, "fleet_loop_advance", None))
    assert callable(getattr(pkg.Solver, "fleet_loop_state", None))
    assert callable(getattr(pkg.closed_loop, "run_lmpc_fleet_fused", None))
    assert callable(getattr(pkg.closed_loop, "run_lmpc_fleet", None))


def test_null_handle_is_an_argument_error(pkg):
    lib = pkg.load_library()
    io = pkg.capi.CFleetLoop()
    assert lib.lmpc_fleet_loop_advance_batch(None, C.c_int32(4), None, C.byref(io)) == -1
    assert lib.lmpc_fleet_loop_advance_batch(None, C.c_int32(4), None, None) == -1


def test_ctypes_mirror_has_the_c_layout(pkg, tmp_path):
    """The struct crosses the ABI by pointer: the mirror's size and the offsets of a member from each run of fields must be the C
    compiler's."""
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    members = ("X_trk", "x", "vel_ref", "dt", "t", "speed_scale", "max_vel_ref_diff", "n_sub", "n_rec", "plant", "phase", "lap_kind",
               "query", "n_fail")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "lmpc_hip.h"\nint main(void) {\n  printf("%zu\\n", sizeof(lmpc_fleet_loop));\n'
                   + "".join('  printf("%%zu\\n", offsetof(lmpc_fleet_loop, %s));\n' % m for m in members) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c11", "-I", str(ROOT / "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    CF = pkg.capi.CFleetLoop
    assert got == [C.sizeof(CF)] + [getattr(CF, m).offset for m in members]
