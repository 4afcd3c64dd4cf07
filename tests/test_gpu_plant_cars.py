"""The car table of include/lmpc_hip_cars.h and lmpc_plant_step_cars_batch: car b stepped by vehicle b, against the oracle's
restatement of the simulator run once per distinct vehicle on that vehicle's cars, and against lmpc_plant_step_batch where every car is
on the handle's vehicle.  B = 70 and B = 300: a full and a partial wave, a full and a partial 256-thread block.  Needs an MI355X."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from oracle import params as P, qp as Q, scenario as S

pytestmark = pytest.mark.gpu

DT_SIM, N_SUB = 0.0125, 2
SLOW, LINE, EULER = 5, 11, (7, 12)   # the car with |vx| < 1e-6, the car within a sub-step of the start line, the two Euler cars


def kinds(base):
    """by b % 3: BARC; mu = 0.7; 20 % less grip and 10 % more mass (tests/test_regression_oracle.py's perturbed plant)"""
    return (dict(base), dict(base, mu=0.7), dict(base, mu=0.8 * base["mu"], m=1.1 * base["m"]))


def oracle_vehicle(d):
    integ = d["integrator"] if isinstance(d["integrator"], str) else ("rk4", "euler")[d["integrator"]]
    return dataclasses.replace(P.barc_vehicle(), mu=d["mu"], m=d["m"], integrator=integ)


@pytest.fixture(scope="module")
def scene(pkg):
    solver = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
    tr = pkg.workloads.synthetic_track("barc")
    trk = solver.device_track(tr)
    cache = {}

    def get(B):
        """states and inputs as tests/test_gpu_path.py's plant check draws them, the two special cars, the table, the oracle's answer"""
        if B not in cache:
            u_lo, u_hi, _, _ = Q.effective_bounds(P.barc_tracking_mpc(20), P.barc_vehicle())
            x, u = pkg.workloads.sample_initial_states("barc", B, tr["L"], u_lo, u_hi, 31)
            x[SLOW, 3] = -3e-7
            x[LINE, 0], x[LINE, 3] = tr["L"] - 0.2 * x[LINE, 3] * DT_SIM, abs(x[LINE, 3])   # crosses the line in its first sub-step
            veh = [kinds(pkg.presets.barc_vehicle())[b % 3] for b in range(B)]
            for b in EULER:
                veh[b] = dict(veh[b], integrator="euler")
            want = np.full((B, 6), np.nan)
            groups = {}
            for b, v in enumerate(veh):
                groups.setdefault((v["mu"], v["m"], v["integrator"]), []).append(b)
            for cars in groups.values():   # the oracle once per distinct vehicle, on that vehicle's cars
                want[cars] = S.plant_step(oracle_vehicle(veh[cars[0]]), tr, x[cars], u[cars], DT_SIM, N_SUB)
            assert len(groups) == 5 and np.isfinite(want).all()
            cache[B] = dict(x=x, u=u, veh=veh, want=want)
        return cache[B]

    yield dict(solver=solver, tr=tr, trk=trk, get=get, pkg=pkg)
    solver.close()


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def step_cars(scene, d, veh=None, order=None, n_sub=N_SUB, launches=1):
    order = np.arange(len(d["veh"])) if order is None else order
    veh = d["veh"] if veh is None else veh
    scene["solver"].set_car_vehicles([veh[b] for b in order])
    xs, ua = dev(d["x"][order].T), dev(d["u"][order].T)
    for _ in range(launches):
        scene["solver"].plant_step_cars(scene["trk"], xs, ua, DT_SIM, n_sub)
    return xs


@pytest.mark.parametrize("B", [70, 300])
def test_each_car_is_stepped_by_its_own_vehicle(scene, B):
    """Against oracle.scenario.plant_step per distinct vehicle, at the bound tests/test_gpu_path.py holds lmpc_plant_step_batch to.
    (Without the car table every car is stepped by one vehicle: two thirds of the cars then miss this bound by seven decades.)"""
    d = scene["get"](B)
    got = step_cars(scene, d).cpu().numpy().T
    want = d["want"]
    err = np.abs(got - want).max()
    print("B = %d: max |device - oracle| = %.3e, bound %.3e" % (B, err, 1e-11 * max(1.0, np.abs(want).max())))
    assert err <= 1e-11 * max(1.0, np.abs(want).max())
    assert (got[:, 0] >= 0).all() and (got[:, 0] < scene["tr"]["L"]).all()
    assert got[LINE, 0] < 0.1 * scene["tr"]["L"] and d["x"][LINE, 0] > 0.9 * scene["tr"]["L"]   # that car did cross the line
    # the cases are what they are meant to be: the vehicles matter far beyond the bound, and so does the integrator
    nominal = S.plant_step(P.barc_vehicle(), scene["tr"], d["x"], d["u"], DT_SIM, N_SUB)
    moved = np.abs(nominal - want).max(axis=1)
    assert (moved[1::3] > 1e-6).all() and (moved[2::3] > 1e-6).all() and (moved[list(EULER)] > 1e-6).all()


@pytest.mark.parametrize("B", [70, 300])
def test_all_cars_on_the_handles_vehicle_is_plant_step(scene, B):
    """Every car on the handle's vehicle: lmpc_plant_step_batch's result within the same bound.  How many values are bit-identical is
    printed -- a finding (profiles/fleet_plants.md), not an assertion: the two kernels inline the model into different code."""
    d = scene["get"](B)
    got = step_cars(scene, d, veh=[scene["pkg"].presets.barc_vehicle()] * B)
    ref, ua = dev(d["x"].T), dev(d["u"].T)
    scene["solver"].plant_step(scene["trk"], ref, ua, DT_SIM, N_SUB)
    want = ref.cpu().numpy()
    same = int((got == ref).sum())
    print("B = %d: %d of %d values bit-identical to lmpc_plant_step_batch, max |difference| %.3e" % (B, same, ref.numel(), np.abs(got.cpu().numpy() - want).max()))
    assert np.abs(got.cpu().numpy() - want).max() <= 1e-11 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("B", [70, 300])
def test_permuting_cars_and_table_permutes_the_result(scene, B):
    import torch
    d = scene["get"](B)
    straight = step_cars(scene, d)
    order = np.random.default_rng(3).permutation(B)
    assert (order != np.arange(B)).sum() > B // 2
    permuted = step_cars(scene, d, order=order)
    assert torch.equal(permuted, straight[:, torch.as_tensor(order, device="cuda")])


@pytest.mark.parametrize("B", [70, 300])
def test_two_launches_of_one_sub_step_are_one_of_two(scene, B):
    import torch
    d = scene["get"](B)
    assert torch.equal(step_cars(scene, d, n_sub=1, launches=2), step_cars(scene, d, n_sub=2))


def test_the_table_reads_back_as_it_was_set(scene):
    d = scene["get"](70)
    scene["solver"].set_car_vehicles(d["veh"])
    back = scene["solver"].car_vehicles()
    assert len(back) == 70
    for b, (got, want) in enumerate(zip(back, d["veh"])):
        want = dict(want, integrator={"rk4": 0, "euler": 1}[want["integrator"]])
        assert got == want, b


def test_refusals_leave_the_state_and_the_table_as_they_were(scene, pkg):
    import torch
    d, s, trk = scene["get"](70), scene["solver"], scene["trk"]
    x0, ua = dev(d["x"].T), dev(d["u"].T)

    def refused(call):
        with pytest.raises(pkg.capi.LmpcError, match=r"-> -1: "):   # LMPC_ERR_ARGUMENT
            call()

    # no table
    s.set_car_vehicles(None)
    xs = x0.clone()
    refused(lambda: s.plant_step_cars(trk, xs, ua, DT_SIM, N_SUB))
    refused(lambda: s.car_vehicles())
    assert torch.equal(xs, x0)
    # a table of 70: another batch
    want = step_cars(scene, d)
    x300, u300 = dev(np.tile(d["x"], (5, 1))[:300].T), dev(np.tile(d["u"], (5, 1))[:300].T)
    keep = x300.clone()
    refused(lambda: s.plant_step_cars(trk, x300, u300, DT_SIM, N_SUB))
    assert torch.equal(x300, keep)
    # a vehicle that is not built: the table in force stays in force
    for bad in (dict(model_id=1), dict(integrator=7)):
        veh = list(d["veh"])
        veh[33] = dict(veh[33], **bad)
        refused(lambda: s.set_car_vehicles(veh))
        refused(lambda: s.set_car_vehicles(veh[:40]))
        xs = x0.clone()
        s.plant_step_cars(trk, xs, ua, DT_SIM, N_SUB)
        assert torch.equal(xs, want)
        assert len(s.car_vehicles()) == 70
    # NULL track, NULL state
    xs = x0.clone()
    ct = s._ctrack(trk)
    for track, xp in ((None, xs.data_ptr()), (C.byref(ct), None)):
        rc = s.lib.lmpc_plant_step_cars_batch(s._h, C.c_int32(70), track, C.c_void_p(xp), C.c_void_p(ua.data_ptr()), C.c_double(DT_SIM), C.c_int32(N_SUB))
        assert rc == -1
    rc = s.lib.lmpc_plant_step_cars_batch(s._h, C.c_int32(70), C.byref(ct), C.c_void_p(xs.data_ptr()), C.c_void_p(ua.data_ptr()), C.c_double(DT_SIM), C.c_int32(0))
    assert rc == -1
    assert torch.equal(xs, x0)
    s.plant_step_cars(trk, xs, ua, DT_SIM, N_SUB)
    assert torch.equal(xs, want)
