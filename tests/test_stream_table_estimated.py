"""tests/test_stream_table.py's lint for include/lmpc_hip_estimated.h: the stream classification of tests/stream_cases_estimated.py
against the prototypes of that header -- its one entry point asynchronous -- so that it cannot ship unclassified or without a row on
the gated stream (tests/test_gpu_streams_estimated.py), and include/lmpc_hip.h includes it behind lmpc_hip_cars_model.h.  No GPU."""
import re
from pathlib import Path

import stream_cases as SC
import stream_cases_cars as SV
import stream_cases_cars_model as SM
import stream_cases_dtrack as SD
import stream_cases_dtrack_model as SDM
import stream_cases_estimated as SE
import stream_cases_fleet_dtrack as SX
import stream_cases_rows as SR
import stream_cases_vanilla_fleet as SF
import test_stream_table as ST
import test_stream_table_cars as STC
import test_stream_table_cars_model as STM
import test_stream_table_dtrack as STD
import test_stream_table_dtrack_model as STDM
import test_stream_table_fleet_dtrack as STX
import test_stream_table_rows as STR
import test_stream_table_vanilla_fleet as STF

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "lmpc_hip_estimated.h"
OTHER_TABLES = (SC, SR, SV, SD, SF, SX, SDM, SM)
NAME = "lmpc_loop_advance_estimated_batch"


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
    assert re.search(r'^#include "lmpc_hip_estimated.h"$', main, flags=re.M)
    # behind lmpc_hip_cars_model.h, inside the extern "C" block
    at = main.index('#include "lmpc_hip_estimated.h"')
    assert main.index('#include "lmpc_hip_cars_model.h"') < at < main.rindex("#ifdef __cplusplus")
    assert main.index('extern "C" {') < at
    _, mine = prototypes()
    assert sorted(mine) == sorted(SE.TABLE)
    for theirs in (STM.prototypes()[1], STDM.prototypes()[1], STX.prototypes()[1], STF.prototypes()[1], STD.prototypes()[1], STC.prototypes()[1],
                   STR.prototypes()[1], ST.prototypes()[1]):
        assert not set(mine) & set(theirs)
    for other in OTHER_TABLES:
        assert not set(SE.TABLE) & set(other.TABLE), other.__name__


def test_the_prototype_is_the_one_the_issue_states():
    _, found = prototypes()
    params = [re.sub(r"\s+", " ", p).strip() for p in found[NAME].split(",")]
    assert params == ["lmpc_handle* h", "int32_t batch", "const lmpc_track* track", "const lmpc_spline_track* spline", "const lmpc_estimated_loop* io"]


def test_every_prototype_has_exactly_one_class():
    _, found = prototypes()
    assert set(found) == set(SE.TABLE), sorted(set(found) ^ set(SE.TABLE))
    for name, (cls, sync, io) in SE.TABLE.items():
        assert cls in (SC.ASYNC, SC.BLOCKING, SC.HOST), name
        assert not (sync and cls != SC.BLOCKING), (name, "only a blocking entry point waits for the stream")
        assert not (io and cls == SC.HOST), (name, "host-only means no device work")
    assert SE.TABLE[NAME] == (SC.ASYNC, False, True)


def test_the_binding_knows_the_same_entry_points(pkg):
    """racing-lmpc-ros2_amd/capi.py resolves this symbol at load time, in a loop of its own: its ninth list is this header's."""
    capi = pkg.capi
    assert set(capi._ABI_SYMBOLS_ESTIMATED) == set(SE.TABLE) and len(capi._ABI_SYMBOLS_ESTIMATED) == len(SE.TABLE)
    assert not set(capi._ABI_SYMBOLS_ESTIMATED) & (set(capi._ABI_SYMBOLS) | set(capi._ABI_SYMBOLS_ROWS) | set(capi._ABI_SYMBOLS_CARS)
                                                   | set(capi._ABI_SYMBOLS_DTRACK) | set(capi._ABI_SYMBOLS_VANILLA_FLEET)
                                                   | set(capi._ABI_SYMBOLS_FLEET_DTRACK) | set(capi._ABI_SYMBOLS_DTRACK_MODEL)
                                                   | set(capi._ABI_SYMBOLS_CARS_MODEL))
    src = (ROOT / "racing-lmpc-ros2_amd" / "capi.py").read_text()
    assert "for sym in _ABI_SYMBOLS_CARS_MODEL:" in src and "for sym in _ABI_SYMBOLS_ESTIMATED:" in src
    lib = pkg.load_library()
    for name in SE.TABLE:
        assert hasattr(lib, name), name


def test_every_entry_point_with_device_work_has_a_row():
    known = set(SE.TABLE) | set(SC.TABLE)
    covered = {f for _, fns in SE.ROWS.values() for f in fns}
    assert covered <= known, sorted(covered - known)
    need = {f for f, (cls, _, io) in SE.TABLE.items() if io}
    assert not sorted(need - covered), "entry points with device inputs, outputs or state and no row: %s" % sorted(need - covered)
    for other in OTHER_TABLES:
        assert not set(SE.ROWS) & set(other.ROWS), other.__name__
    for row, (_, fns) in SE.ROWS.items():
        cls, sync = SE.row_class(row)
        assert cls == (SC.BLOCKING if any(SE.entry(f)[0] == SC.BLOCKING for f in fns) else SC.ASYNC), row
        assert sync == any(SE.entry(f)[1] for f in fns), row
        assert (cls, sync) == (SC.ASYNC, False), row


def test_the_header_says_what_the_table_says():
    """The entry point is not blocking: no sentence of the header says that it synchronises, waits for or blocks on a stream
    (test_stream_table.says_it_waits over every comment of the header); the comment in front of it calls it asynchronous and not
    host-only."""
    text, _ = prototypes()
    comments = [m.group(0) for m in re.finditer(r"/\*.*?\*/", text, flags=re.S)]
    for name, (cls, sync, _) in SE.TABLE.items():
        assert not sync
        assert not ST.says_it_waits(name, comments, comments), (name, "a comment of the header says that it waits for the stream")
    blank = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), text, flags=re.S)
    found = list(re.finditer(r"/\*.*?\*/", text, flags=re.S))
    at = re.search(r"\b%s\s*\(" % NAME, blank).start()
    front = [m.group(0) for m in found if m.end() <= at][-1]
    assert "Host-only" not in front and "asynchronous" in front
