"""The C ABI of include/lmpc_hip_vanilla_fleet.h without a GPU: its one symbol is exported and declared, lmpc_vanilla_fleet_rollout
has the size and the fields the header states, lmpc_hip.h includes the header behind the lmpc_vanilla_* prototypes, a null handle is
refused, and the header is pedantic C11."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "lmpc_hip_vanilla_fleet.h"
SYMBOLS = ("lmpc_vanilla_rollout_fleet_batch",)


def test_the_symbol_is_declared_and_exported(pkg):
    code = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lmpc_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(SYMBOLS)
    lib = pkg.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert tuple(pkg.capi._ABI_SYMBOLS_VANILLA_FLEET) == SYMBOLS


def test_struct_size_and_layout(pkg):
    capi = pkg.capi
    text = HEADER.read_text()
    stated = int(re.search(r"\} lmpc_vanilla_fleet_rollout; /\* sizeof == (\d+) \*/", text).group(1))
    assert C.sizeof(capi.CVanillaFleetRollout) == stated == 112
    m = re.search(r"typedef struct lmpc_vanilla_fleet_rollout \{(.*?)\} lmpc_vanilla_fleet_rollout;", text, flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n.strip(" *") for line in re.findall(r"\b(?:double|int32_t|int64_t)\s*\*?\s*([^;]+);", body) for n in line.split(",")]
    assert names == [n for n, _ in capi.CVanillaFleetRollout._fields_]
    # the constants of the binding are the header's
    defs = dict(re.findall(r"#define (LMPC_VANILLA_(?:PLANT|RECORD)_\w+)\s+(\d+)", text))
    assert {k: int(v) for k, v in defs.items()} == {
        "LMPC_VANILLA_PLANT_HANDLE": capi.VANILLA_PLANT["handle"], "LMPC_VANILLA_PLANT_CARS": capi.VANILLA_PLANT["cars"],
        "LMPC_VANILLA_PLANT_DTRACK": capi.VANILLA_PLANT["dtrack"], "LMPC_VANILLA_RECORD_NONE": capi.VANILLA_RECORD[None],
        "LMPC_VANILLA_RECORD_APPLIED": capi.VANILLA_RECORD["applied"], "LMPC_VANILLA_RECORD_ARRIVED": capi.VANILLA_RECORD["arrived"]}


def test_the_main_header_includes_it_behind_the_vanilla_prototypes():
    main = (ROOT / "include" / "lmpc_hip.h").read_text()
    at = main.index('#include "lmpc_hip_vanilla_fleet.h"')
    assert main.index("int lmpc_vanilla_rollout_batch(") < at < main.index("#ifdef __cplusplus\n}")
    assert at > main.index('#include "lmpc_hip_dtrack.h"')
    assert not re.search(r"lmpc_vanilla_rollout_fleet_batch\s*\(", main), "the prototype belongs to lmpc_hip_vanilla_fleet.h"
    guard = HEADER.read_text()
    assert "#ifndef LMPC_HIP_H_\n#error" in guard


def test_a_null_handle_is_an_argument_error(pkg):
    lib = pkg.load_library()
    io = pkg.capi.CVanillaFleetRollout()
    assert lib.lmpc_vanilla_rollout_fleet_batch(None, C.c_int32(1), None, None, C.byref(io)) == -1
    assert lib.lmpc_vanilla_rollout_fleet_batch(None, C.c_int32(1), None, None, None) == -1


def test_header_is_pedantic_c11(pkg, tmp_path):
    """tests/test_abi.py's gcc line on a caller of the entry point."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "vf.c"
    src.write_text(r'''
#include <stddef.h>
#include "lmpc_hip.h"
int run(lmpc_handle* h, int B, const lmpc_spline_track* sp, lmpc_track table, double* x, double* u_prev) {
  lmpc_vanilla_fleet_rollout io = {0};
  io.x = x;
  io.u_prev = u_prev;
  io.periods = 64;
  io.n_sub = 2;
  io.plant = LMPC_VANILLA_PLANT_DTRACK;
  io.record = LMPC_VANILLA_RECORD_ARRIVED;
  io.dt_sim = 0.0125;
  io.speed_scale = 1.0;
  io.period0 = 64;
  io.dt = 0.025;
  return lmpc_vanilla_rollout_fleet_batch(h, B, sp, &table, &io);
}
int main(void) {
  return (sizeof(lmpc_vanilla_fleet_rollout) == 112 && lmpc_vanilla_rollout_fleet_batch(NULL, 1, NULL, NULL, NULL) == LMPC_ERR_ARGUMENT) ? 0 : 1;
}
''')
    lib = Path(pkg.capi.library_path()).resolve()
    assert lib.exists()
    exe = tmp_path / "vf"
    r = subprocess.run([gcc, "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(exe),
                        f"-L{lib.parent}", "-llmpc_hip", f"-Wl,-rpath,{lib.parent}", "-Wl,--allow-shlib-undefined"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
