"""The numpy restatement of lmpc_vanilla_rollout_fleet_batch (tests/vanilla_fleet_cases.py) held to what it is built from, the
qualification gate the device tests of tests/test_gpu_vanilla_fleet.py rely on, and the measurement its double-track tolerance comes
from.  No GPU."""
import math

import numpy as np
import pytest

import vanilla_cases as VC
import vanilla_fleet_cases as FC

GATE_B, GATE_PERIODS, LAPS_WANTED = 16, 1000, 2


def test_on_the_handles_vehicle_it_is_the_vanilla_rollout(pkg):
    """Every car on the handle's vehicle, by the handle's plant and through the car table's path: vanilla_cases.rollout, bit for bit,
    and u_prev is the last logged input."""
    sc = VC.scenario("barc")
    ref = VC.reference("barc", "rollout", VC.PERIODS)
    args = (sc["veh"], sc["cfg"], sc["trk"], sc["x0"], VC.zero_pid(VC.B_TEST), VC.PERIODS, sc["dt_sim"], sc["n_sub"], sc["speed_scale"])
    for kw in (dict(plant="handle"), dict(plant="cars", vehicles=FC.car_vehicles(sc, VC.B_TEST, mixed=False))):
        got = FC.rollout(*args, **kw)
        for k in VC.ROLLOUT_KEYS + ("flags",):
            assert np.array_equal(got[k], ref[k]), (kw["plant"], k)
        assert all(np.array_equal(got["pid"][k], ref["pid"][k]) for k in VC.PID_KEYS)
        assert np.array_equal(got["u_prev"], ref["U_log"][:, :, -1])
    mixed = FC.reference(pkg, "cars")
    assert VC.err(mixed["x"], ref["x"]) > 1e-6, "the mixed car table drives the scenario's laps: nothing to tell apart"


def test_the_two_conventions_record_the_same_states_and_shifted_inputs(pkg):
    sc = VC.scenario("barc", GATE_B)
    laps = {}
    for record in ("applied", "arrived"):
        fleet = FC.HostFleet(pkg, GATE_B, 512)
        FC.rollout(sc["veh"], sc["cfg"], sc["trk"], sc["x0"], VC.zero_pid(GATE_B), 400, sc["dt_sim"], sc["n_sub"], sc["speed_scale"],
                   record=record, fleet=fleet, period0=7, dt=sc["dt"], u_prev=np.full((GATE_B, 2), 0.5))
        laps[record] = [fleet.laps(b) for b in range(GATE_B)]
    n = 0
    for a, r in zip(laps["applied"], laps["arrived"]):
        assert len(a) == len(r)
        for (ax, au, ak, at), (rx, ru, rk, rt) in zip(a, r):
            assert np.array_equal(ax, rx) and np.array_equal(ak, rk) and np.array_equal(at, rt)
            assert np.array_equal(au[:-1], ru[1:])          # the input applied from sample j is the one that led to sample j + 1
            assert np.allclose(np.diff(at), sc["dt"], rtol=0, atol=1e-12)
            n += 1
    assert n >= 1


@pytest.mark.parametrize("plant", FC.PLANTS)
def test_qualification_gate(pkg, plant):
    """What every device test of the recorder relies on, B = 16 and 1000 periods of the BARC scenario on each plant: no car frozen,
    no body over an edge, at least two closed laps per car, every lap within 512 samples, and with slots of 256 every lap overflows."""
    sc = VC.scenario("barc", GATE_B)
    vehicles = None if plant == "handle" else FC.car_vehicles(sc, GATE_B) if plant == "cars" else FC.dtrack_vehicles(pkg, GATE_B)
    big, small = FC.HostFleet(pkg, GATE_B, 512), FC.HostFleet(pkg, GATE_B, 256)

    class Both:
        def step(self, *a):
            big.step(*a)
            small.step(*a)

    got = FC.rollout(sc["veh"], sc["cfg"], sc["trk"], sc["x0"], VC.zero_pid(GATE_B), GATE_PERIODS, sc["dt_sim"], sc["n_sub"], sc["speed_scale"],
                     plant=plant, vehicles=vehicles, record="arrived", fleet=Both(), dt=sc["dt"], u_prev=np.zeros((GATE_B, 2)))
    st, st_small = big.stats(), small.stats()
    lengths = [n for b in range(GATE_B) for n in big.lap_lengths(b)]
    print(plant, "worst_excess %.4f, laps per car %d .. %d, samples per lap %d .. %d"
          % (got["worst_excess"].max(), st["laps_in_ring"].min(), st["laps_in_ring"].max(), min(lengths), max(lengths)))
    assert not got["flags"].any()
    assert (got["worst_excess"] <= 0.0).all()
    assert (st["laps_in_ring"] >= LAPS_WANTED).all() and (st["lap_count"] >= LAPS_WANTED + 1).all()
    assert max(lengths) <= 512 and not st["n_dropped"].any()
    assert not st_small["laps_in_ring"].any() and np.array_equal(st_small["n_dropped"], st["lap_count"] - 1)
    if plant == "cars":
        assert all(v.integrator == "euler" for b, v in enumerate(vehicles) if b in FC.EULER) and len(FC.EULER) == 2


def test_double_track_rollout_tolerance_is_the_measured_one(pkg):
    """The restatement with the closed-form gamma_y root against the same restatement with the kernel's five Newton iterations, over
    exactly the 64 periods and 67 cars of the device test: the drift rounded up to a power of ten is TOL_TWIN_DTRACK, and the device
    tolerance is 1e4 times that -- vanilla_cases.TOL_ROLLOUT's rule -- and at most 1e-8."""
    closed = FC.reference(pkg, "dtrack")
    sc = VC.scenario("barc")
    with FC.newton_gamma():
        newton = FC.rollout(sc["veh"], sc["cfg"], sc["trk"], sc["x0"], VC.zero_pid(VC.B_TEST), VC.PERIODS, sc["dt_sim"], sc["n_sub"],
                            sc["speed_scale"], plant="dtrack", vehicles=FC.dtrack_vehicles(pkg, VC.B_TEST))
    assert FC.DC.gamma_closed_form is not FC.gamma_newton
    assert not closed["flags"].any() and not newton["flags"].any()
    worst = {k: VC.err(newton[k], closed[k]) for k in VC.ROLLOUT_KEYS}
    worst["pid"] = max(VC.err(newton["pid"][k], closed["pid"][k]) for k in VC.PID_KEYS)
    drift = max(worst.values())
    print("closed form against Newton, 64 periods:", {k: "%.1e" % v for k, v in worst.items()})
    assert 0.0 < drift <= FC.TOL_TWIN_DTRACK
    assert FC.TOL_TWIN_DTRACK == 10.0 ** math.ceil(math.log10(drift)), "TOL_TWIN_DTRACK is the drift rounded up to a power of ten"
    assert FC.TOL_DTRACK == 1e4 * FC.TOL_TWIN_DTRACK <= 1e-8
    # the four-wheel fleet is another plant, not the single-track one with other numbers
    assert VC.err(closed["x"], VC.reference("barc", "rollout", VC.PERIODS)["x"]) > 1e-6
