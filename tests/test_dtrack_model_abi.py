"""The C ABI of include/lmpc_hip_dtrack_model.h without a GPU: its three symbols are exported and declared there and nowhere else,
lmpc_hip.h includes the header behind lmpc_hip_fleet_dtrack.h, a null handle is refused, the header is pedantic C11 with a caller of
the three, and the binding and the closed loops carry the feature."""
import ctypes as C
import inspect
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "lmpc_hip_dtrack_model.h"
SYMBOLS = ("lmpc_linearize_dtrack_batch", "lmpc_dtrack_set_controller_model", "lmpc_dtrack_get_controller_model")


def test_the_three_symbols_are_declared_here_only_and_exported(pkg):
    code = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lmpc_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(SYMBOLS)
    lib = pkg.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert tuple(pkg.capi._ABI_SYMBOLS_DTRACK_MODEL) == SYMBOLS
    for other in sorted((ROOT / "include").glob("*.h")):
        if other != HEADER:
            text = re.sub(r"/\*.*?\*/", "", other.read_text(), flags=re.S)
            for name in SYMBOLS:
                assert not re.search(r"\b%s\s*\(" % name, text), (other.name, name, "the prototype belongs to lmpc_hip_dtrack_model.h")
    assert "#ifndef LMPC_HIP_H_\n#error" in HEADER.read_text()


def test_the_main_header_includes_it_behind_the_fused_period():
    main = (ROOT / "include" / "lmpc_hip.h").read_text()
    at = main.index('#include "lmpc_hip_dtrack_model.h"')
    assert main.index('#include "lmpc_hip_fleet_dtrack.h"') < at < main.rindex("#ifdef __cplusplus")
    between = main[main.index('#include "lmpc_hip_fleet_dtrack.h"'):at]
    assert between.count("#include") == 1, "nothing else is included between the two"
    # the adjacency the older headers' tests hold
    assert '#include "lmpc_hip_rows.h"\n#include "lmpc_hip_cars.h"\n#include "lmpc_hip_dtrack.h"\n' in main


def test_a_null_handle_is_an_argument_error(pkg):
    lib = pkg.load_library()
    on = C.c_int32(7)
    assert lib.lmpc_linearize_dtrack_batch(None, C.c_int32(1), None, None, None, None, None, None, None) == -1
    assert lib.lmpc_dtrack_set_controller_model(None, C.c_int32(1)) == -1
    assert lib.lmpc_dtrack_set_controller_model(None, C.c_int32(0)) == -1
    assert lib.lmpc_dtrack_get_controller_model(None, C.byref(on)) == -1 and on.value == 7


def test_solver_and_closed_loops_carry_it(pkg):
    S = pkg.Solver
    assert list(inspect.signature(S.linearize_dtrack).parameters)[:2] == ["self", "inp"]
    assert list(inspect.signature(S.set_dtrack_controller_model).parameters) == ["self", "on"]
    assert isinstance(S.dtrack_controller_model, property) and S.dtrack_controller_model.fset is None
    for fn in (pkg.closed_loop.run_lmpc_fleet, pkg.closed_loop.run_lmpc_fleet_fused):
        assert inspect.signature(fn).parameters["controllers_dt"].default is None


def test_header_is_pedantic_c11(pkg, tmp_path):
    """tests/test_abi.py's gcc line on a caller of the three entry points."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "dm.c"
    src.write_text(r'''
#include <stddef.h>
#include "lmpc_hip.h"
int run(lmpc_handle* h, int B, lmpc_vehicle_dt* veh, const double* X, const double* U, const double* T, const double* k, double* A,
        double* Bm, double* g) {
  int32_t on = 0;
  int rc = lmpc_dtrack_set_vehicles(h, B, veh);
  if (rc == LMPC_OK) rc = lmpc_linearize_dtrack_batch(h, B, X, U, T, k, A, Bm, g);
  if (rc == LMPC_OK) rc = lmpc_dtrack_set_controller_model(h, 1);
  if (rc == LMPC_OK) rc = lmpc_dtrack_get_controller_model(h, &on);
  return rc == LMPC_OK ? on : rc;
}
int main(void) {
  int32_t on = 0;
  return (lmpc_linearize_dtrack_batch(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == LMPC_ERR_ARGUMENT &&
          lmpc_dtrack_set_controller_model(NULL, 1) == LMPC_ERR_ARGUMENT && lmpc_dtrack_get_controller_model(NULL, &on) == LMPC_ERR_ARGUMENT)
             ? 0
             : 1;
}
''')
    lib = Path(pkg.capi.library_path()).resolve()
    assert lib.exists()
    exe = tmp_path / "dm"
    r = subprocess.run([gcc, "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(exe),
                        f"-L{lib.parent}", "-llmpc_hip", f"-Wl,-rpath,{lib.parent}", "-Wl,--allow-shlib-undefined"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
