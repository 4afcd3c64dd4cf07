"""The entry point of include/lmpc_hip_fleet_dtrack.h held to its stream contract on a gated stream: tests/test_gpu_streams.py's
check for the row of tests/stream_cases_fleet_dtrack.py, by the model of tests/test_gpu_streams_vanilla_fleet.py and with its gate.
The row runs on the default stream (the reference) and on a fresh non-blocking stream behind a finite delay, with another valid draw
in the input buffers until the stream itself copies the real inputs in: the results -- state, u_prev, references, the loop's state,
accumulators, gamma_y, the recorders' counters and the rings -- are the reference's bit for bit, and the call has returned while the
gate still held the stream.  Needs an MI355X."""
import pytest

import stream_cases as SC
import stream_cases_fleet_dtrack as SX
import test_gpu_fleet_loop as FL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rows(pkg):
    built = SX.build(pkg)
    refs = {row: SC.reference(case) for row, case in built.items()}
    gate = SC.Gate()
    slow = max(sec for r, (_, sec) in refs.items() if SX.row_class(r)[0] == SC.ASYNC)
    gate_ms = max(SC.GATE_FACTOR * slow * 1e3, SC.GATE_FLOOR_MS)
    measured = gate.tune(gate_ms)
    assert measured >= gate_ms >= SC.GATE_FLOOR_MS, (measured, gate_ms)
    yield dict(built=built, refs=refs, gate=gate, gate_ms=gate_ms)
    # the scene is test_gpu_fleet_loop's cache: the table this module set is cleared, and what it added to the cache is closed
    for sc in FL._scenes.values():
        sc["learner"].set_dtrack_vehicles(None)
        for sv in (sc["tracker"], sc["learner"], sc["ref"], *sc["plants"].values()):
            sv.close()
    FL._scenes.clear()


@pytest.mark.parametrize("row", list(SX.ROWS))
def test_row_on_a_gated_stream(rows, row):
    case = rows["built"][row]
    want, _ = rows["refs"][row]
    got, closed = SC.gated(case, rows["gate"], rows["gate_ms"])
    diff = SC.differences(got, want)
    assert not diff, (row, "differs from the default-stream run in", diff)
    assert case.cls == SC.ASYNC
    assert closed, (row, "returned after the gate had opened: a synchronisation the header denies (or a host call slower than the gate)")
    # the equality is not vacuous: the other filling of the buffers gives another result
    assert SC.differences(SC.reference(case, "stale")[0], want), (row, "`stale` gives the result of `real`: the row would prove nothing")


def test_the_plant_ran(rows):
    """gamma_y came from the call (the sentinel is gone) and the cars moved."""
    want, _ = rows["refs"]["fleet_loop_advance_dtrack"]
    case = rows["built"]["fleet_loop_advance_dtrack"]
    g = want["out gamma_y"].cpu().numpy()
    assert (g != SC.SENTINEL_F).all() and abs(g).max() > 0
    assert bool((want["in place x"] != case.real["x"]).any(dim=0).all())
