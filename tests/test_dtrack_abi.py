"""The C ABI of include/lmpc_hip_dtrack.h without a GPU: its three symbols are exported and declared, lmpc_vehicle_dt has the size the
header states, lmpc_hip.h includes the header where it says, a null handle is refused, the header is pedantic C11, and the presets
and the parameter loader give the fields the struct takes."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "lmpc_hip_dtrack.h"
SYMBOLS = ("lmpc_dtrack_set_vehicles", "lmpc_dtrack_get_vehicles", "lmpc_plant_step_dtrack_batch")


def test_the_three_symbols_are_declared_and_exported(pkg):
    code = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lmpc_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(SYMBOLS)
    lib = pkg.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert tuple(pkg.capi._ABI_SYMBOLS_DTRACK) == SYMBOLS


def test_struct_size_and_layout(pkg):
    capi = pkg.capi
    assert C.sizeof(capi.CVehicleDT) == 280 == 8 + 34 * 8
    assert capi.CVehicleDT.base.offset == 0 and capi.CVehicleDT.tw_f.offset == C.sizeof(capi.CVehicle)
    m = re.search(r"typedef struct lmpc_vehicle_dt \{(.*?)\} lmpc_vehicle_dt;", HEADER.read_text(), flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n.strip() for line in re.findall(r"\bdouble\s+([^;]+);", body) for n in line.split(",")]
    assert ["base"] + names == [n for n, _ in capi.CVehicleDT._fields_]


def test_the_main_header_includes_it_right_after_the_car_table():
    main = (ROOT / "include" / "lmpc_hip.h").read_text()
    assert '#include "lmpc_hip_cars.h"\n#include "lmpc_hip_dtrack.h"\n' in main
    assert not re.search(r"lmpc_dtrack_\w+\s*\(|lmpc_plant_step_dtrack_batch\s*\(", main), "the prototypes belong to lmpc_hip_dtrack.h"


def test_a_null_handle_is_an_argument_error(pkg):
    lib = pkg.load_library()
    assert lib.lmpc_dtrack_set_vehicles(None, C.c_int32(0), None) == -1
    assert lib.lmpc_dtrack_get_vehicles(None, C.c_int32(1), None) == -1
    assert lib.lmpc_plant_step_dtrack_batch(None, C.c_int32(1), None, None, None, C.c_double(0.01), C.c_int32(1), None) == -1


def test_header_is_pedantic_c11(pkg, tmp_path):
    """tests/test_abi.py's gcc line on a caller of the three entry points."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "dt.c"
    src.write_text(r'''
#include <stddef.h>
#include "lmpc_hip.h"
int run(lmpc_handle* h, int B, lmpc_track track, lmpc_vehicle_dt* veh, double* x, const double* u, double* gamma_y) {
  int rc = lmpc_dtrack_set_vehicles(h, B, veh);
  if (rc == LMPC_OK) rc = lmpc_plant_step_dtrack_batch(h, B, &track, x, u, 0.0125, 2, gamma_y);
  if (rc == LMPC_OK) rc = lmpc_dtrack_get_vehicles(h, B, veh);
  return rc;
}
int main(void) {
  return (sizeof(lmpc_vehicle_dt) == 8 + 34 * 8 && LMPC_DTRACK_NEWTON >= 1 && lmpc_dtrack_set_vehicles(NULL, 0, NULL) == LMPC_ERR_ARGUMENT) ? 0 : 1;
}
''')
    lib = Path(pkg.capi.library_path()).resolve()
    assert lib.exists()
    exe = tmp_path / "dt"
    r = subprocess.run([gcc, "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(exe),
                        f"-L{lib.parent}", "-llmpc_hip", f"-Wl,-rpath,{lib.parent}", "-Wl,--allow-shlib-undefined"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_presets_and_loader_agree_with_the_committed_parameter_files(pkg, tmp_path):
    """presets.*_double_track are the single-track presets plus the extras of the base files; the loader reads the same files and a
    double_track_planar.* file beside them."""
    R, PS = pkg.ros_params, pkg.presets
    extra = tmp_path / "double_track.param.yaml"
    fields = [n for n, _ in pkg.capi.CVehicle._fields_] + [n for n, _ in pkg.capi.CVehicleDT._fields_[1:]]
    for car, single, double in (("barc", PS.barc_vehicle(), PS.barc_double_track()), ("iac_car", PS.iac_vehicle(), PS.iac_double_track())):
        assert sorted(double) == sorted(fields)
        assert double["model_id"] == 2 and double["kroll_f"] == 0.5
        assert {k: v for k, v in double.items() if k in single and k != "model_id"} == {k: v for k, v in single.items() if k != "model_id"}
        extra.write_text("/**:\n  ros__parameters:\n    double_track_planar:\n      fd_max: %r\n      fb_max: %r\n      td: %r\n      tb: %r\n"
                         "      v_max: 100.0\n      p_max: 1.0e6\n      kroll_f: 0.5\n      mu: %r\n"
                         % (single["Fd_max"], single["Fb_max"], single["Td"], single["Tb"], single["mu"]))
        base = ROOT / "tests" / "golden" / "ros_params" / car / (car + "_base.param.yaml")
        params = R.load_ros_params(base, extra)
        assert R.double_track_vehicle_from_params(params) == double
        with pytest.raises(KeyError, match="double_track_planar.kroll_f"):
            R.double_track_vehicle_from_params({k: v for k, v in params.items() if k != "double_track_planar.kroll_f"})
    assert "double_track_vehicle_from_params" in R.__all__
