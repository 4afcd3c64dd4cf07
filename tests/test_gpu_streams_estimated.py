"""The entry point of include/lmpc_hip_estimated.h held to its stream contract on a gated stream: tests/test_gpu_streams.py's check for
the row of tests/stream_cases_estimated.py.  The row runs on the default stream (the reference) and on a fresh non-blocking stream
behind a finite delay, with another valid draw in the input buffers until the stream itself copies the real inputs in: every output,
every array updated in place and the filter's store are the reference's bit for bit, and the call has returned while the gate still
held the stream.  The gate is sized as there: 10 times the slowest ungated host time of a row of this module, 20 ms at least.  Needs
an MI355X."""
import pytest

import stream_cases as SC
import stream_cases_estimated as SE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rows(pkg):
    built = SE.build(pkg)
    refs = {row: SC.reference(case) for row, case in built.items()}
    gate = SC.Gate()
    slow = max(sec for r, (_, sec) in refs.items() if SE.row_class(r)[0] == SC.ASYNC)
    gate_ms = max(SC.GATE_FACTOR * slow * 1e3, SC.GATE_FLOOR_MS)
    measured = gate.tune(gate_ms)
    assert measured >= gate_ms >= SC.GATE_FLOOR_MS, (measured, gate_ms)
    yield dict(built=built, refs=refs, gate=gate, gate_ms=gate_ms)
    for case in built.values():
        for sv in (case.keep if isinstance(case.keep, tuple) else (case.keep,)):
            if hasattr(sv, "close"):
                sv.close()


@pytest.mark.parametrize("row", list(SE.ROWS))
def test_row_on_a_gated_stream(rows, row):
    case = rows["built"][row]
    want, _ = rows["refs"][row]
    got, closed = SC.gated(case, rows["gate"], rows["gate_ms"])
    diff = SC.differences(got, want)
    assert not diff, (row, "differs from the default-stream run in", diff)
    assert case.cls == SC.ASYNC and not case.sync
    assert closed, (row, "returned after the gate had opened: a synchronisation the header denies (or a host call slower than the gate)")
    # the equality is not vacuous: the other filling of the buffers gives another result
    assert SC.differences(SC.reference(case, "stale")[0], want), (row, "`stale` gives the result of `real`: the row would prove nothing")
