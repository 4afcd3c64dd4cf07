"""The C ABI of include/lmpc_hip_fleet_dtrack.h: its one symbol is exported and declared there and nowhere else, lmpc_fleet_loop is
the size it was (the entry point adds no member to it), a null handle is refused, the header is pedantic C11 -- all without a GPU --
and, on one (a handle cannot be made without a device), the two refusals that need a handle and nothing else: no fleet store, and a
NULL io."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "lmpc_hip_fleet_dtrack.h"
SYMBOLS = ("lmpc_fleet_loop_advance_dtrack_batch",)
# sizeof(lmpc_fleet_loop) as tests/test_fleet_loop_abi.py holds it to the C compiler on the parent of this entry point, counted from
# the header's member list: 15 pointers, 3 + 3 x 2 doubles, 6 int32, the plant pointer, 10 pointers
FLEET_LOOP_BYTES = 15 * 8 + 9 * 8 + 6 * 4 + 8 + 10 * 8
assert FLEET_LOOP_BYTES == 304


def test_the_symbol_is_declared_and_exported(pkg):
    code = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lmpc_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(SYMBOLS)
    lib = pkg.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert tuple(pkg.capi._ABI_SYMBOLS_FLEET_DTRACK) == SYMBOLS
    main = (ROOT / "include" / "lmpc_hip.h").read_text()
    assert not re.search(r"lmpc_fleet_loop_advance_dtrack_batch\s*\(", main), "the prototype belongs to lmpc_hip_fleet_dtrack.h"
    assert "#ifndef LMPC_HIP_H_\n#error" in HEADER.read_text()


def test_lmpc_fleet_loop_is_the_size_it_was(pkg, tmp_path):
    assert C.sizeof(pkg.capi.CFleetLoop) == FLEET_LOOP_BYTES
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        return      # (the mirror is held to the compiler by tests/test_fleet_loop_abi.py where there is one)
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "lmpc_hip.h"\nint main(void) {\n  printf("%zu\\n", sizeof(lmpc_fleet_loop));\n  return 0;\n}\n')
    exe = tmp_path / "size"
    subprocess.check_call([cc, "-std=c11", "-I", str(ROOT / "include"), "-o", str(exe), str(src)])
    assert int(subprocess.check_output([str(exe)])) == FLEET_LOOP_BYTES


def test_solver_and_closed_loop_carry_it(pkg):
    import inspect
    sig = inspect.signature(pkg.Solver.fleet_loop_advance)
    assert sig.parameters["dtrack"].default is False and sig.parameters["gamma_y"].default is None
    assert inspect.signature(pkg.closed_loop.run_lmpc_fleet_fused).parameters["plants_dt"].default is None


def test_a_null_handle_is_an_argument_error(pkg):
    lib = pkg.load_library()
    io = pkg.capi.CFleetLoop()
    assert lib.lmpc_fleet_loop_advance_dtrack_batch(None, C.c_int32(4), None, C.byref(io), None) == -1
    assert lib.lmpc_fleet_loop_advance_dtrack_batch(None, C.c_int32(4), None, None, None) == -1


def test_header_is_pedantic_c11(pkg, tmp_path):
    """tests/test_abi.py's gcc line on a caller of the entry point."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "fd.c"
    src.write_text(r'''
#include <stddef.h>
#include "lmpc_hip.h"
int run(lmpc_handle* h, int B, lmpc_track table, lmpc_fleet_loop io, double* gamma_y) {
  io.plant = NULL;
  return lmpc_fleet_loop_advance_dtrack_batch(h, B, &table, &io, gamma_y);
}
int main(void) {
  return (sizeof(lmpc_fleet_loop) == 304 && lmpc_fleet_loop_advance_dtrack_batch(NULL, 1, NULL, NULL, NULL) == LMPC_ERR_ARGUMENT) ? 0 : 1;
}
''')
    lib = Path(pkg.capi.library_path()).resolve()
    assert lib.exists()
    exe = tmp_path / "fd"
    r = subprocess.run([gcc, "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(exe),
                        f"-L{lib.parent}", "-llmpc_hip", f"-Wl,-rpath,{lib.parent}", "-Wl,--allow-shlib-undefined"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.gpu
def test_refusals_that_need_only_a_handle(pkg):
    """A handle without a fleet store, and a NULL io: LMPC_ERR_ARGUMENT with a message in lmpc_last_error."""
    lib = pkg.load_library()
    solver = pkg.Solver(pkg.presets.barc_lmpc(20, 2), pkg.presets.barc_vehicle(), device=0)
    try:
        trk = solver.device_track(pkg.workloads.synthetic_track("barc"))
        ct = solver._ctrack(trk)
        io = pkg.capi.CFleetLoop()
        for arg in (C.byref(io), None):
            assert lib.lmpc_fleet_loop_advance_dtrack_batch(solver._h, C.c_int32(4), C.byref(ct), arg, None) == -1
            assert len(lib.lmpc_last_error(solver._h) or b"") > 0
    finally:
        solver.close()
