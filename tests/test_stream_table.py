"""The stream classification of tests/stream_cases.py against the prototypes of include/lmpc_hip.h: a new entry point cannot ship
unclassified, and one with device inputs or outputs cannot ship without a row on the gated stream (tests/test_gpu_streams.py).
No GPU."""
import re
from pathlib import Path

import stream_cases as SC

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "lmpc_hip.h"


def prototypes():
    """name -> (the comment block in front of the prototype's group, the parameter list), comments and preprocessor lines aside."""
    text = HEADER.read_text()
    code = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), text, flags=re.S)      # same offsets: the comments are looked up below
    code = re.sub(r"^[ \t]*#.*$", lambda m: " " * len(m.group(0)), code, flags=re.M)
    found = {}
    for m in re.finditer(r"\b(?:int|void|const\s+char\s*\*)\s+(lmpc_\w+)\s*\(([^;{}]*?)\)\s*;", code, flags=re.S):
        assert m.group(1) not in found, m.group(1)
        found[m.group(1)] = m.group(2)
    return text, found


def test_every_prototype_has_exactly_one_class():
    _, found = prototypes()
    assert len(found) >= 77, sorted(found)          # the parser sees the header (77 entry points when this test was written)
    missing = sorted(set(found) - set(SC.TABLE))
    extra = sorted(set(SC.TABLE) - set(found))
    assert not missing, "entry points without a stream class in tests/stream_cases.py TABLE: %s" % missing
    assert not extra, "TABLE names functions the header does not declare: %s" % extra
    for name, (cls, sync, io) in SC.TABLE.items():
        assert cls in (SC.ASYNC, SC.BLOCKING, SC.HOST), name
        assert not (sync and cls != SC.BLOCKING), (name, "only a blocking entry point waits for the stream")
        assert not (io and cls == SC.HOST), (name, "host-only means no device work")


def test_the_binding_knows_the_same_entry_points():
    """racing-lmpc-ros2_amd/capi.py resolves every symbol at load time: its list is the header's."""
    src = (ROOT / "racing-lmpc-ros2_amd" / "capi.py").read_text()
    block = src[src.index("_ABI_SYMBOLS = ("):]
    names = set(re.findall(r'"(lmpc_\w+)"', block[:block.index(")")]))
    assert names == set(SC.TABLE), sorted(names ^ set(SC.TABLE))


def test_every_entry_point_with_device_work_has_a_row():
    covered = {f for _, fns in SC.ROWS.values() for f in fns}
    assert covered <= set(SC.TABLE), sorted(covered - set(SC.TABLE))
    assert not [f for f in covered if SC.TABLE[f][0] == SC.HOST], "a host-only entry point needs no row"
    need = {f for f, (cls, _, io) in SC.TABLE.items() if io}
    assert not sorted(need - covered), "entry points with device inputs, outputs or state and no row: %s" % sorted(need - covered)
    assert {g for g, _ in SC.ROWS.values()} == set(SC.BUILDERS)
    for row, (_, fns) in SC.ROWS.items():
        cls, sync = SC.row_class(row)
        assert cls == (SC.BLOCKING if any(SC.TABLE[f][0] == SC.BLOCKING for f in fns) else SC.ASYNC), row
        assert sync == any(SC.TABLE[f][1] for f in fns), row


def test_pointer_arguments_mean_device_work():
    """A prototype that takes a data pointer beside the handle -- anything but the handle, a config / spec / track struct, a string
    or a host scalar result -- is not host-only unless it is one of the few that only record or report a host value."""
    _, found = prototypes()
    host_values = {"lmpc_last_error", "lmpc_set_stream", "lmpc_set_launch_order", "lmpc_query_launch", "lmpc_query_residency",
                   "lmpc_query_launch_for", "lmpc_last_solve_precision", "lmpc_fleet_ss_bytes"}
    for name, params in found.items():
        data = [p for p in params.split(",") if re.search(r"\b(double|float|int32_t|int64_t|uint64_t)\s*\*", p)]
        if data and SC.TABLE[name][0] == SC.HOST:
            assert name in host_values, (name, data)


WAITS = re.compile(r"synchronis|\bwaits?\b|Block until", re.I)
DENIES = re.compile(r"\b(neither|nor|not|never|no|without)\b[^.;]*?(synchronis|\bwaits?\b)", re.I)


def sentences(comment: str):
    body = re.sub(r"\s*\n\s*\*\s?", " ", comment.strip("/*"))
    return [s.strip() for s in re.split(r"(?<=\.)\s+", body) if s.strip()]


def says_it_waits(name: str, own: list, others: list) -> bool:
    """A sentence that says so and does not deny it: in the comment directly in front of (or behind) the prototype where that sentence
    names no other entry point, or anywhere in the header where the sentence names this one."""
    def good(s):
        return bool(WAITS.search(s)) and not DENIES.search(s)

    for c in own:
        for s in sentences(c):
            named = set(re.findall(r"lmpc_\w+", s))
            if good(s) and (not named or name in named):
                return True
    return any(good(s) and name in re.findall(r"lmpc_\w+", s) for c in others for s in sentences(c))


def test_the_header_says_what_the_table_says():
    """The words the classes are taken from: every entry point marked `sync` has a sentence of its own that says it synchronises,
    waits for or blocks on the handle's stream (says_it_waits); the asynchronous ones are under the header's general rule."""
    text, _ = prototypes()
    assert "goes to the handle's stream (lmpc_set_stream)" in text and "is ASYNCHRONOUS unless its comment says" in text
    blank = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), text, flags=re.S)
    comments = [m for m in re.finditer(r"/\*.*?\*/", text, flags=re.S)]
    for name, (cls, sync, _) in SC.TABLE.items():
        if not sync:
            continue
        at = re.search(r"\b%s\s*\(" % name, blank).start()
        end = text.index(";", at)
        line_end = text.index("\n", end)
        front = [m.group(0) for m in comments if m.end() <= at][-1:]
        # (a comment inside the parameter list or behind the prototype on its line)
        inline = [m.group(0) for m in comments if at < m.start() < line_end]
        others = [m.group(0) for m in comments if m.group(0) not in front + inline]
        assert says_it_waits(name, front + inline, others), (name, "no sentence of the header says that it waits for the stream")


def test_the_lint_holds_the_sentence_to_the_function():
    assert says_it_waits("lmpc_a", ["/* Uploads once and synchronises the handle's stream. */"], [])
    assert not says_it_waits("lmpc_a", ["/* Enqueues and neither waits for the stream nor reads it. */"], [])
    assert not says_it_waits("lmpc_a", ["/* Asynchronous; lmpc_b waits for the handle's stream. */"], [])
    assert says_it_waits("lmpc_a", [], ["/* Something else.  lmpc_a and lmpc_b wait... no: lmpc_a waits for the stream. */"])
    assert not says_it_waits("lmpc_a", [], ["/* lmpc_b synchronises the handle's stream. */"])
