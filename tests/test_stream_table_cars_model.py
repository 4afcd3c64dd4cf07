"""tests/test_stream_table.py's lint for include/lmpc_hip_cars_model.h: the stream classification of tests/stream_cases_cars_model.py
against the prototypes of that header -- the linearisation asynchronous, the two switch functions host-only -- so that its entry
points cannot ship unclassified or without a row on the gated stream (tests/test_gpu_streams_cars_model.py), and include/lmpc_hip.h
includes it behind lmpc_hip_dtrack_model.h.  No GPU."""
import re
from pathlib import Path

import stream_cases as SC
import stream_cases_cars as SV
import stream_cases_cars_model as SM
import stream_cases_dtrack as SD
import stream_cases_dtrack_model as SDM
import stream_cases_fleet_dtrack as SX
import stream_cases_rows as SR
import stream_cases_vanilla_fleet as SF
import test_stream_table as ST
import test_stream_table_cars as STC
import test_stream_table_dtrack as STD
import test_stream_table_dtrack_model as STDM
import test_stream_table_fleet_dtrack as STX
import test_stream_table_rows as STR
import test_stream_table_vanilla_fleet as STF

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "lmpc_hip_cars_model.h"
OTHER_TABLES = (SC, SR, SV, SD, SF, SX, SDM)


def prototypes():
    """name -> parameter list, by test_stream_table.prototypes' expression."""
    text = HEADER.read_text()
    code = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), text, flags=re.S)
    code = re.sub(r"^[ \t]*#.*$", lambda m: " " * len(m.group(0)), code, flags=re.M)
    found = {}
    for m in re.finditer(r"\b(?:int|void|const\s+char\s*\*)\s+(lmpc_\w+)\s*\(([^;{}]*?)\)\s*;", code, flags=re.S):
        assert m.group(1) not in found, m.group(1)
        found[m.group(1)] = m.group(2)
    return text, found


def test_the_main_header_includes_this_one_and_no_name_is_declared_twice():
    main = (ROOT / "include" / "lmpc_hip.h").read_text()
    assert re.search(r'^#include "lmpc_hip_cars_model.h"$', main, flags=re.M)
    # behind lmpc_hip_dtrack_model.h (and so behind the table's header), inside the extern "C" block; the adjacency of the rows / cars /
    # dtrack includes stands
    at = main.index('#include "lmpc_hip_cars_model.h"')
    assert main.index('#include "lmpc_hip_dtrack_model.h"') < at < main.rindex("#ifdef __cplusplus")
    assert main.index('#include "lmpc_hip_cars.h"') < at
    assert main.index('extern "C" {') < at
    assert '#include "lmpc_hip_rows.h"\n#include "lmpc_hip_cars.h"\n#include "lmpc_hip_dtrack.h"\n' in main
    _, mine = prototypes()
    assert sorted(mine) == sorted(SM.TABLE)
    for theirs in (STDM.prototypes()[1], STX.prototypes()[1], STF.prototypes()[1], STD.prototypes()[1], STC.prototypes()[1], STR.prototypes()[1],
                   ST.prototypes()[1]):
        assert not set(mine) & set(theirs)
    for other in OTHER_TABLES:
        assert not set(SM.TABLE) & set(other.TABLE), other.__name__


def test_the_prototypes_are_the_ones_the_issue_states():
    _, found = prototypes()
    params = {n: [re.sub(r"\s+", " ", p).strip() for p in found[n].split(",")] for n in found}
    assert params["lmpc_linearize_cars_batch"] == ["lmpc_handle* h", "int32_t batch", "const double* X_ref", "const double* U_ref",
                                                   "const double* T_ref", "const double* curvatures", "double* A", "double* Bm", "double* g"]
    assert params["lmpc_cars_set_controller_model"] == ["lmpc_handle* h", "int32_t on"]
    assert params["lmpc_cars_get_controller_model"] == ["const lmpc_handle* h", "int32_t* on"]
    # modelled on the double-track header: the same parameter lists, name for name
    theirs = STDM.prototypes()[1]
    for mine, other in (("lmpc_linearize_cars_batch", "lmpc_linearize_dtrack_batch"), ("lmpc_cars_set_controller_model", "lmpc_dtrack_set_controller_model"),
                        ("lmpc_cars_get_controller_model", "lmpc_dtrack_get_controller_model")):
        assert params[mine] == [re.sub(r"\s+", " ", p).strip() for p in theirs[other].split(",")], mine


def test_every_prototype_has_exactly_one_class():
    _, found = prototypes()
    assert set(found) == set(SM.TABLE), sorted(set(found) ^ set(SM.TABLE))
    for name, (cls, sync, io) in SM.TABLE.items():
        assert cls in (SC.ASYNC, SC.BLOCKING, SC.HOST), name
        assert not (sync and cls != SC.BLOCKING), (name, "only a blocking entry point waits for the stream")
        assert not (io and cls == SC.HOST), (name, "host-only means no device work")
    assert SM.TABLE["lmpc_linearize_cars_batch"] == (SC.ASYNC, False, True)
    assert SM.TABLE["lmpc_cars_set_controller_model"] == (SC.HOST, False, False)
    assert SM.TABLE["lmpc_cars_get_controller_model"] == (SC.HOST, False, False)


def test_the_binding_knows_the_same_entry_points(pkg):
    """racing-lmpc-ros2_amd/capi.py resolves these symbols at load time, in a loop of their own: its eighth list is this header's."""
    capi = pkg.capi
    assert set(capi._ABI_SYMBOLS_CARS_MODEL) == set(SM.TABLE) and len(capi._ABI_SYMBOLS_CARS_MODEL) == len(SM.TABLE)
    assert not set(capi._ABI_SYMBOLS_CARS_MODEL) & (set(capi._ABI_SYMBOLS) | set(capi._ABI_SYMBOLS_ROWS) | set(capi._ABI_SYMBOLS_CARS)
                                                    | set(capi._ABI_SYMBOLS_DTRACK) | set(capi._ABI_SYMBOLS_VANILLA_FLEET)
                                                    | set(capi._ABI_SYMBOLS_FLEET_DTRACK) | set(capi._ABI_SYMBOLS_DTRACK_MODEL))
    src = (ROOT / "racing-lmpc-ros2_amd" / "capi.py").read_text()
    assert "for sym in _ABI_SYMBOLS_DTRACK_MODEL:" in src and "for sym in _ABI_SYMBOLS_CARS_MODEL:" in src
    lib = pkg.load_library()
    for name in SM.TABLE:
        assert hasattr(lib, name), name


def test_every_entry_point_with_device_work_has_a_row():
    known = set(SM.TABLE) | set(SC.TABLE)
    covered = {f for _, fns in SM.ROWS.values() for f in fns}
    assert covered <= known, sorted(covered - known)
    need = {f for f, (cls, _, io) in SM.TABLE.items() if io}
    assert not sorted(need - covered), "entry points with device inputs, outputs or state and no row: %s" % sorted(need - covered)
    # the switch is host-only and needs no row of its own; it has two all the same, in front of the fp64 and the single-precision solve
    # it redirects
    assert sum("lmpc_cars_set_controller_model" in fns for _, fns in SM.ROWS.values()) == 2
    assert {"lmpc_solve_batch", "lmpc_solve_batch_f32"} <= covered
    for other in OTHER_TABLES:
        assert not set(SM.ROWS) & set(other.ROWS), other.__name__
    for row, (_, fns) in SM.ROWS.items():
        cls, sync = SM.row_class(row)
        assert cls == (SC.BLOCKING if any(SM.entry(f)[0] == SC.BLOCKING for f in fns) else SC.ASYNC), row
        assert sync == any(SM.entry(f)[1] for f in fns), row
        assert (cls, sync) == (SC.ASYNC, False), row


def test_the_header_says_what_the_table_says():
    """No entry point of this header is blocking: no sentence of it says that one synchronises, waits for or blocks on a stream
    (test_stream_table.says_it_waits over every comment of the header); the two switch functions are called host-only in the comment
    in front of them, and the linearisation is not."""
    text, _ = prototypes()
    comments = [m.group(0) for m in re.finditer(r"/\*.*?\*/", text, flags=re.S)]
    for name, (cls, sync, _) in SM.TABLE.items():
        assert not sync
        assert not ST.says_it_waits(name, comments, comments), (name, "a comment of the header says that it waits for the stream")
    blank = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), text, flags=re.S)
    found = list(re.finditer(r"/\*.*?\*/", text, flags=re.S))
    for name, (cls, _, _) in SM.TABLE.items():
        at = re.search(r"\b%s\s*\(" % name, blank).start()
        front = [m.group(0) for m in found if m.end() <= at][-1]
        assert ("Host-only" in front) == (cls == SC.HOST), name
