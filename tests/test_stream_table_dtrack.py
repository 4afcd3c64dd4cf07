"""tests/test_stream_table.py's lint for include/lmpc_hip_dtrack.h: the stream classification of tests/stream_cases_dtrack.py against
the prototypes of that header, so that its entry points cannot ship unclassified or without a row on the gated stream
(tests/test_gpu_streams_dtrack.py), and include/lmpc_hip.h includes it.  No GPU."""
import re
from pathlib import Path

import stream_cases as SC
import stream_cases_cars as SV
import stream_cases_dtrack as SD
import stream_cases_rows as SR
import test_stream_table as ST
import test_stream_table_cars as STC
import test_stream_table_rows as STR

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "lmpc_hip_dtrack.h"


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
    assert re.search(r'^#include "lmpc_hip_dtrack.h"$', main, flags=re.M)
    # right after the include of lmpc_hip_cars.h, and behind every type its prototypes name
    assert '#include "lmpc_hip_cars.h"\n#include "lmpc_hip_dtrack.h"\n' in main
    _, mine = prototypes()
    others = [STC.prototypes()[1], STR.prototypes()[1], ST.prototypes()[1]]
    assert len(mine) == 3, sorted(mine)
    for theirs in others:
        assert not set(mine) & set(theirs)
    assert not set(SD.TABLE) & (set(SC.TABLE) | set(SR.TABLE) | set(SV.TABLE))


def test_every_prototype_has_exactly_one_class():
    _, found = prototypes()
    assert set(found) == set(SD.TABLE), sorted(set(found) ^ set(SD.TABLE))
    for name, (cls, sync, io) in SD.TABLE.items():
        assert cls in (SC.ASYNC, SC.BLOCKING, SC.HOST), name
        assert not (sync and cls != SC.BLOCKING), (name, "only a blocking entry point waits for the stream")
        assert not (io and cls == SC.HOST), (name, "host-only means no device work")
    assert SD.TABLE["lmpc_dtrack_set_vehicles"] == (SC.BLOCKING, True, True)
    assert SD.TABLE["lmpc_dtrack_get_vehicles"] == (SC.BLOCKING, True, True)
    assert SD.TABLE["lmpc_plant_step_dtrack_batch"] == (SC.ASYNC, False, True)


def test_the_binding_knows_the_same_entry_points(pkg):
    """racing-lmpc-ros2_amd/capi.py resolves these symbols at load time, in a loop of their own: its fourth list is this header's, and
    the loops over the first three stand as tests/test_stream_table_rows.py and tests/test_stream_table_cars.py read them."""
    capi = pkg.capi
    assert set(capi._ABI_SYMBOLS_DTRACK) == set(SD.TABLE) and len(capi._ABI_SYMBOLS_DTRACK) == len(SD.TABLE)
    assert not set(capi._ABI_SYMBOLS_DTRACK) & (set(capi._ABI_SYMBOLS) | set(capi._ABI_SYMBOLS_ROWS) | set(capi._ABI_SYMBOLS_CARS))
    src = (ROOT / "racing-lmpc-ros2_amd" / "capi.py").read_text()
    assert "for sym in _ABI_SYMBOLS_CARS:" in src and "for sym in _ABI_SYMBOLS_DTRACK:" in src
    lib = pkg.load_library()
    for name in SD.TABLE:
        assert hasattr(lib, name), name


def test_every_entry_point_with_device_work_has_a_row():
    known = set(SD.TABLE) | set(SC.TABLE)
    covered = {f for _, fns in SD.ROWS.values() for f in fns}
    assert covered <= known, sorted(covered - known)
    assert not [f for f in covered if SD.entry(f)[0] == SC.HOST], "a host-only entry point needs no row"
    need = {f for f, (cls, _, io) in SD.TABLE.items() if io}
    assert not sorted(need - covered), "entry points with device inputs, outputs or state and no row: %s" % sorted(need - covered)
    assert not set(SD.ROWS) & (set(SC.ROWS) | set(SR.ROWS) | set(SV.ROWS))
    for row, (_, fns) in SD.ROWS.items():
        cls, sync = SD.row_class(row)
        assert cls == (SC.BLOCKING if any(SD.entry(f)[0] == SC.BLOCKING for f in fns) else SC.ASYNC), row
        assert sync == any(SD.entry(f)[1] for f in fns), row


def test_the_header_says_what_the_table_says():
    """Every entry point marked `sync` has a sentence of its own, in this header, that says it synchronises the handle's stream
    (test_stream_table.says_it_waits); the asynchronous one has none that says so."""
    text, _ = prototypes()
    blank = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), text, flags=re.S)
    comments = list(re.finditer(r"/\*.*?\*/", text, flags=re.S))
    for name, (cls, sync, _) in SD.TABLE.items():
        at = re.search(r"\b%s\s*\(" % name, blank).start()
        line_end = text.index("\n", text.index(";", at))
        front = [m.group(0) for m in comments if m.end() <= at][-1:]
        inline = [m.group(0) for m in comments if at < m.start() < line_end]
        others = [m.group(0) for m in comments if m.group(0) not in front + inline]
        if sync:
            assert ST.says_it_waits(name, front + inline, others), (name, "no sentence of the header says that it waits for the stream")
        else:
            assert not ST.says_it_waits(name, front + inline, []), (name, "its own comment says that it waits for the stream")
