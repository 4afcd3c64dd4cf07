"""tests/test_stream_table.py's lint for include/lmpc_hip_fleet_dtrack.h: the stream classification of
tests/stream_cases_fleet_dtrack.py against the prototype of that header, so that its entry point cannot ship unclassified or without
a row on the gated stream (tests/test_gpu_streams_fleet_dtrack.py), and include/lmpc_hip.h includes it.  No GPU."""
import re
from pathlib import Path

import stream_cases as SC
import stream_cases_cars as SV
import stream_cases_dtrack as SD
import stream_cases_fleet_dtrack as SX
import stream_cases_rows as SR
import stream_cases_vanilla_fleet as SF
import test_stream_table as ST
import test_stream_table_cars as STC
import test_stream_table_dtrack as STD
import test_stream_table_rows as STR
import test_stream_table_vanilla_fleet as STF

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "lmpc_hip_fleet_dtrack.h"
NAME = "lmpc_fleet_loop_advance_dtrack_batch"


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
    assert re.search(r'^#include "lmpc_hip_fleet_dtrack.h"$', main, flags=re.M)
    # behind lmpc_fleet_loop and lmpc_hip_dtrack.h -- the types and the table its prototype names -- and inside the extern "C" block
    at = main.index('#include "lmpc_hip_fleet_dtrack.h"')
    assert main.index("} lmpc_fleet_loop;") < at < main.rindex("#ifdef __cplusplus")
    assert main.index('#include "lmpc_hip_dtrack.h"') < at
    assert main.index('extern "C" {') < at
    _, mine = prototypes()
    others = [STF.prototypes()[1], STD.prototypes()[1], STC.prototypes()[1], STR.prototypes()[1], ST.prototypes()[1]]
    assert sorted(mine) == [NAME]
    for theirs in others:
        assert not set(mine) & set(theirs)
    assert not set(SX.TABLE) & (set(SC.TABLE) | set(SR.TABLE) | set(SV.TABLE) | set(SD.TABLE) | set(SF.TABLE))


def test_the_prototype_is_the_one_the_issue_states():
    _, found = prototypes()
    params = [re.sub(r"\s+", " ", p).strip() for p in found[NAME].split(",")]
    assert params == ["lmpc_handle* h", "int32_t batch", "const lmpc_track* track", "const lmpc_fleet_loop* io", "double* gamma_y_or_null"]


def test_every_prototype_has_exactly_one_class():
    _, found = prototypes()
    assert set(found) == set(SX.TABLE), sorted(set(found) ^ set(SX.TABLE))
    for name, (cls, sync, io) in SX.TABLE.items():
        assert cls in (SC.ASYNC, SC.BLOCKING, SC.HOST), name
        assert not (sync and cls != SC.BLOCKING), (name, "only a blocking entry point waits for the stream")
        assert not (io and cls == SC.HOST), (name, "host-only means no device work")
    assert SX.TABLE[NAME] == (SC.ASYNC, False, True)


def test_the_binding_knows_the_same_entry_points(pkg):
    """racing-lmpc-ros2_amd/capi.py resolves this symbol at load time, in a loop of its own: its sixth list is this header's, and the
    loops over the first five stand as the tests of the other headers read them."""
    capi = pkg.capi
    assert set(capi._ABI_SYMBOLS_FLEET_DTRACK) == set(SX.TABLE) and len(capi._ABI_SYMBOLS_FLEET_DTRACK) == len(SX.TABLE)
    assert not set(capi._ABI_SYMBOLS_FLEET_DTRACK) & (set(capi._ABI_SYMBOLS) | set(capi._ABI_SYMBOLS_ROWS) | set(capi._ABI_SYMBOLS_CARS)
                                                      | set(capi._ABI_SYMBOLS_DTRACK) | set(capi._ABI_SYMBOLS_VANILLA_FLEET))
    src = (ROOT / "racing-lmpc-ros2_amd" / "capi.py").read_text()
    assert "for sym in _ABI_SYMBOLS_VANILLA_FLEET:" in src and "for sym in _ABI_SYMBOLS_FLEET_DTRACK:" in src
    lib = pkg.load_library()
    for name in SX.TABLE:
        assert hasattr(lib, name), name


def test_every_entry_point_with_device_work_has_a_row():
    known = set(SX.TABLE) | set(SC.TABLE)
    covered = {f for _, fns in SX.ROWS.values() for f in fns}
    assert covered <= known, sorted(covered - known)
    assert not [f for f in covered if SX.entry(f)[0] == SC.HOST], "a host-only entry point needs no row"
    need = {f for f, (cls, _, io) in SX.TABLE.items() if io}
    assert not sorted(need - covered), "entry points with device inputs, outputs or state and no row: %s" % sorted(need - covered)
    assert not set(SX.ROWS) & (set(SC.ROWS) | set(SR.ROWS) | set(SV.ROWS) | set(SD.ROWS) | set(SF.ROWS))
    for row, (_, fns) in SX.ROWS.items():
        cls, sync = SX.row_class(row)
        assert cls == (SC.BLOCKING if any(SX.entry(f)[0] == SC.BLOCKING for f in fns) else SC.ASYNC), row
        assert sync == any(SX.entry(f)[1] for f in fns), row


def test_the_header_says_nothing_about_waiting():
    """The entry point is asynchronous: no sentence of this header says that it synchronises, waits for or blocks on a stream
    (test_stream_table.says_it_waits over every comment of the header)."""
    text, _ = prototypes()
    comments = [m.group(0) for m in re.finditer(r"/\*.*?\*/", text, flags=re.S)]
    for name, (cls, sync, _) in SX.TABLE.items():
        assert not sync
        assert not ST.says_it_waits(name, comments, comments), (name, "a comment of the header says that it waits for the stream")
