"""The entry points of include/lmpc_hip_dtrack.h held to their stream contract on a gated stream: tests/test_gpu_streams.py's check
for the rows of tests/stream_cases_dtrack.py.  Each row runs on the default stream (the reference) and on a fresh non-blocking stream
behind a finite delay, with another valid draw in the input buffers until the stream itself copies the real inputs in: the results
are the reference's bit for bit, the asynchronous row has returned while the gate still held the stream, and a row with an entry
point whose comment says that it synchronises the handle's stream has not.  The gate is sized as there: 10 times the slowest
ungated host time of an asynchronous row of this module, 20 ms at least.  Needs an MI355X."""
import pytest

import stream_cases as SC
import stream_cases_dtrack as SD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rows(pkg):
    built = SD.build(pkg)
    refs = {row: SC.reference(case) for row, case in built.items()}
    gate = SC.Gate()
    slow = max(sec for r, (_, sec) in refs.items() if SD.row_class(r)[0] == SC.ASYNC)
    gate_ms = max(SC.GATE_FACTOR * slow * 1e3, SC.GATE_FLOOR_MS)
    measured = gate.tune(gate_ms)
    assert measured >= gate_ms >= SC.GATE_FLOOR_MS, (measured, gate_ms)
    yield dict(built=built, refs=refs, gate=gate, gate_ms=gate_ms)
    for case in built.values():
        for sv in (case.keep if isinstance(case.keep, tuple) else (case.keep,)):
            if hasattr(sv, "close"):
                sv.close()


@pytest.mark.parametrize("row", list(SD.ROWS))
def test_row_on_a_gated_stream(rows, row):
    case = rows["built"][row]
    want, _ = rows["refs"][row]
    got, closed = SC.gated(case, rows["gate"], rows["gate_ms"])
    diff = SC.differences(got, want)
    assert not diff, (row, "differs from the default-stream run in", diff)
    if case.cls == SC.ASYNC:
        assert closed, (row, "returned after the gate had opened: a synchronisation the header denies (or a host call slower than the gate)")
    elif case.sync:
        assert not closed, (row, "returned while the gate still held the stream it says it waits for")
    # the equality is not vacuous: the other filling of the buffers gives another result
    assert SC.differences(SC.reference(case, "stale")[0], want), (row, "`stale` gives the result of `real`: the row would prove nothing")


def test_the_table_is_in_effect(rows, pkg):
    """The rows step three kinds of four-wheel car: with every car on the preset the cars of the two other kinds get other bits, and
    the single-track lmpc_plant_step_batch on the same states gives other bits on every car."""
    case = rows["built"]["plant_step_dtrack"]
    want, _ = rows["refs"]["plant_step_dtrack"]
    one = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
    trk = one.device_track(pkg.workloads.synthetic_track("barc"))
    bufs = SC.like(case.real)
    one.set_dtrack_vehicles([pkg.presets.barc_double_track()] * SC.B)
    one.plant_step_dtrack(trk, bufs["x"], bufs["u"], SC.DT / 2, 2)
    same = (bufs["x"] == want["in place x"]).all(dim=0).cpu().numpy()
    assert same[0::3].all() and not same[1::3].any() and not same[2::3].any()
    bufs = SC.like(case.real)
    one.plant_step(trk, bufs["x"], bufs["u"], SC.DT / 2, 2)
    assert not (bufs["x"] == want["in place x"]).all(dim=0).any()
    one.close()
