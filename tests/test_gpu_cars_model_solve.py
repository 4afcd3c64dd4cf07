"""GPU: solves with the per-car controller model switched on (include/lmpc_hip_cars_model.h), against the DENSE optimum of the QP built
on PER-CAR stage models of the oracle (tests/cars_model_cases.py FIXTURES, tests/golden/dense_cars_*.npz: rk4_jacobian_analytic with car
b's Vehicle + oracle.qp.build_qp(cfg, handle_vehicle, lin=...), never the product's linearisation).  What this pins that the
operation-level test (tests/test_gpu_cars_model.py, the separate A / Bm / g arrays) cannot: the kernel's write into the solve's
linearisation records, read by the one-wave kernel (N = 20), by the two-wave kernel's own loader (N = 41, N = 40 at IAC scale), by the
learning kernel and, through the float instantiation, by the single-precision kernel.

With the switch off the same call misses every fixture optimum by more than MIN_DISTANCE = 1e-4: the fixtures tell a controller that
knows its car from one that does not, and the test fails without the feature.  Then every interlock of the header, and one closed loop:
8 different cars driven by controllers that know them."""
import numpy as np
import pytest
import torch

import cars_model_cases as MC
import stream_cases as SC
from parity import per_problem_err
from tolerances import TOL_DU, TOL_F32, TOL_XU

pytestmark = pytest.mark.gpu
GOLD = MC.__file__.rsplit("/", 1)[0] + "/golden"
S345 = (3, 4, 5)
ROWS = {3: (S345, (0,)), 4: (S345, (1,)), 5: (S345, (1,))}


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items() if hasattr(v, "cpu")}


@pytest.fixture(scope="module")
def cases(pkg):
    """fixture, inputs and a handle with the fixture's table, per name; built on first use, closed at the end"""
    made = {}

    def get(name):
        if name not in made:
            with np.load(f"{GOLD}/dense_{name}.npz") as z:
                fx = {k: z[k] for k in z.files}
            cfg, veh, inp, ss_x, ss_j, table = MC.build(pkg, name)
            np.testing.assert_allclose(MC.DC.digest(inp, ss_x, ss_j), fx["digest"], rtol=1e-11, atol=0)
            assert (fx["status"] == 0).all() and fx["status"].size == MC.FIXTURES[name][2]
            sv = pkg.Solver(*MC.presets(pkg, name), device=0)
            sv.set_car_vehicles(table)
            ss = None if ss_x is None else (torch.as_tensor(ss_x, device="cuda"), torch.as_tensor(ss_j, device="cuda"))
            made[name] = dict(fx=fx, inp=inp, sv=sv, ss=ss, B=fx["status"].size, table=table)
        return made[name]

    yield get
    for c in made.values():
        c["sv"].close()


def solve(c, on, mixed=False, warm=None):
    sv = c["sv"]
    sv.set_cars_controller_model(on)
    assert sv.cars_controller_model == on
    if c["ss"] is None:
        return _np(sv.solve(c["inp"], mixed=mixed, warm=warm))
    o = sv.alloc_outputs(c["B"])
    o["convex_combi_optm"] = torch.zeros((c["ss"][0].shape[1], c["B"]), dtype=torch.float64, device="cuda")
    return _np(sv.solve(c["inp"], o, ss_x=c["ss"][0], ss_j=c["ss"][1], mixed=mixed, warm=warm))


@pytest.mark.parametrize("name", list(MC.FIXTURES))
def test_solve_on_each_cars_own_vehicle_against_the_dense_optimum(cases, name):
    """lmpc_solve_batch with the switch on: status 0 on every problem, X / U / dU within TOL_XU / TOL_DU (scaled) of the fixture optimum
    (for the learning set too: the weights are compared as tests/test_gpu_dense_fixtures.py compares them, through the states and
    inputs they produce).  The same call with the switch off misses the fixture by more than MIN_DISTANCE on every problem."""
    c = cases(name)
    out = solve(c, True)
    assert (out["status"] == 0).all(), (name, np.nonzero(out["status"])[0], out["status"][out["status"] != 0])
    exu, ed = per_problem_err(out, c["fx"])
    off = solve(c, False)
    oxu, od = per_problem_err(off, c["fx"])
    miss = np.maximum(oxu, od)
    print("%s: %d problems, kernel vs dense X/U max %.1e median %.1e, dU max %.1e, iterations mean %.2f; switch off: misses the fixture by "
          "min %.1e max %.1e" % (name, exu.size, exu.max(), np.median(exu), ed.max(), out["iters"].mean(), miss.min(), miss.max()))
    assert exu.max() < TOL_XU and ed.max() < TOL_DU, (name, np.argsort(np.maximum(exu, ed))[-3:], exu.max(), ed.max())
    assert (miss > MC.MIN_DISTANCE).all(), (name, "the solve on the handle's vehicle is this close to the per-car optimum", miss.min(), int(np.argmin(miss)))


def test_mixed_and_warm_entries_on_each_cars_own_vehicle(cases):
    """cars_trk_n20 through lmpc_solve_batch_mixed (TOL_F32 against the dense optimum, tests/tolerances.py) and through
    lmpc_solve_batch_warm with the cold solution as the plan: the same answer within the contract, accepted somewhere."""
    c = cases("cars_trk_n20")
    sv = c["sv"]
    mixed = solve(c, True, mixed=True)
    assert sv.last_solve_precision() == "mixed"
    assert (mixed["status"] == 0).all(), np.nonzero(mixed["status"])[0]
    exu, ed = per_problem_err(mixed, c["fx"])
    print("cars_trk_n20 mixed: X/U max %.1e median %.1e, dU max %.1e" % (exu.max(), np.median(exu), ed.max()))
    assert exu.max() < TOL_F32 and ed.max() < TOL_F32 / 0.025, (exu.max(), ed.max())
    cold = solve(c, True)
    plan = {"X_optm_ref": torch.as_tensor(cold["X_optm"], device="cuda"), "U_optm_ref": torch.as_tensor(cold["U_optm"], device="cuda")}
    warm = solve(c, True, warm=plan)
    accepted = sv.warm_accepted(c["B"]).cpu().numpy()
    assert (warm["status"] == 0).all()
    wxu, wd = per_problem_err(warm, c["fx"])
    print("cars_trk_n20 warm: X/U max %.1e, dU max %.1e; accepted %d of %d, iterations mean %.2f (cold %.2f)"
          % (wxu.max(), wd.max(), accepted.sum(), accepted.size, warm["iters"].mean(), cold["iters"].mean()))
    assert wxu.max() < TOL_XU and wd.max() < TOL_DU
    assert accepted.any()
    # the warm entry with the switch off lands on the other optimum: the switch reaches this entry too
    off = solve(c, False, warm=plan)
    oxu, od = per_problem_err(off, c["fx"])
    assert (np.maximum(oxu, od) > MC.MIN_DISTANCE).all()
    off = solve(c, False, mixed=True)
    oxu, od = per_problem_err(off, c["fx"])
    assert (np.maximum(oxu, od) > MC.MIN_DISTANCE).all()


def test_single_precision_entry_on_each_cars_own_vehicle(cases):
    """cars_iac_n40 through lmpc_solve_batch_f32: the float instantiation of the kernel (fp64 arithmetic on car b's vehicle, float
    records) in front of the single-precision QP kernel, within TOL_F32 of the dense optimum; with the switch off the same call misses
    every problem by more than MIN_DISTANCE."""
    c = cases("cars_iac_n40")
    sv = c["sv"]
    got = {}
    for on in (True, False):
        sv.set_cars_controller_model(on)
        out = _np(sv.solve_f32(c["inp"]))
        assert sv.last_solve_precision() == "f32"
        assert (out["status"] == 0).all(), (on, np.nonzero(out["status"])[0])
        exu, ed = per_problem_err({k: out[k].astype(np.float64) for k in ("X_optm", "U_optm", "dU_optm")}, c["fx"])
        got[on] = (exu, ed)
    exu, ed = got[True]
    miss = np.maximum(*got[False])
    print("cars_iac_n40 f32: X/U max %.1e median %.1e, dU max %.1e; switch off: misses the fixture by min %.1e max %.1e"
          % (exu.max(), np.median(exu), ed.max(), miss.min(), miss.max()))
    assert exu.max() < TOL_F32 and ed.max() < TOL_F32 / 0.025, (exu.max(), ed.max())
    assert (miss > MC.MIN_DISTANCE).all(), miss.min()


def test_host_entry_solves_on_vehicle_0_of_a_table_of_one(cases, pkg):
    """lmpc_solve_host is a batch of one: with a table of one vehicle it solves problem 0 of the fixture on that vehicle; with the
    fixture's table of 48 it is refused."""
    c = cases("cars_trk_n20")
    inp9 = {k: torch.as_tensor(c["inp"][k], device="cuda") for k in SC.KEYS9}
    hx = SC._host_problem(inp9, 0)
    L = float(pkg.workloads.synthetic_track("barc")["L"])
    sv = pkg.Solver(*MC.presets(pkg, "cars_trk_n20"), device=0)
    sv.set_car_vehicles(c["table"])
    sv.set_cars_controller_model(True)
    with pytest.raises(pkg.capi.LmpcError, match=r"-> -1: "):
        SC._solve_host(sv, L, hx)
    sv.set_car_vehicles(c["table"][:1])
    assert sv.cars_controller_model, "replacing the table keeps the switch on"
    on = SC._solve_host(sv, L, hx)
    sv.set_cars_controller_model(False)
    off = SC._solve_host(sv, L, hx)
    sv.close()
    want = {k: c["fx"][k][..., :1] for k in ("X_optm", "U_optm", "dU_optm")}
    as_batch = lambda r: {"X_optm": r["X"].T[..., None], "U_optm": r["U"].T[..., None], "dU_optm": r["dU"].T[..., None]}   # noqa: E731
    assert on["status"][0] == 0 and off["status"][0] == 0
    exu, ed = per_problem_err(as_batch(on), want)
    oxu, od = per_problem_err(as_batch(off), want)
    print("lmpc_solve_host on vehicle 0: X/U %.1e dU %.1e; switch off: %.1e" % (exu.max(), ed.max(), max(oxu.max(), od.max())))
    assert exu.max() < TOL_XU and ed.max() < TOL_DU
    assert max(oxu.max(), od.max()) > MC.MIN_DISTANCE


def _cold(pkg, s, B, seed):
    tr = pkg.workloads.synthetic_track("barc")
    trk = s.device_track(tr)
    L = float(tr["L"])
    return dict(SC._cold_inputs(pkg, s, trk, L, seed, n=B), L=L)


def _solve(s, inp, **kw):
    out = s.solve(inp, SC._solve_outs(s, inp["x_ic"].shape[1]), **kw)
    return {k: v for k, v in out.items() if hasattr(v, "cpu")}


def test_interlocks_and_refusals(pkg):
    """Every interlock of the header: the switch against each of the four regressions, in both orders; against the double-track switch,
    in both orders; the sequential-QP entry; a batch other than the table's through every batched entry, with the pre-filled outputs
    untouched; and freeing the table, which switches the model off -- after which a solve is the solve of a handle that never had it
    on."""
    B = 70
    s = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
    inp = _cold(pkg, s, B, 22)
    veh = MC.fleet(pkg.presets.barc_vehicle(), B)

    def refused(code, call):
        with pytest.raises(pkg.capi.LmpcError, match=r"-> %d: " % code):
            call()

    refused(-1, lambda: s.set_cars_controller_model(True))   # no table
    assert not s.cars_controller_model
    s.set_car_vehicles(veh)
    x, u = pkg.workloads.sample_initial_states("barc", 6, inp["L"], [-0.01, -0.3], [0.01, 0.3], seed=9)
    laps = [(x, u, np.zeros(6), 0.03 * np.arange(6))]
    s.fleet_ss_create(B, 64)
    regressions = {
        "shared": (lambda: s.set_regression_laps(laps, dist_max=0.6), lambda: s.set_regression_laps([])),
        "shared, per row": (lambda: s.set_regression_laps(laps, rows=ROWS, dist_max=0.6), lambda: s.set_regression_laps([])),
        "per car": (lambda: s.fleet_ss_set_regression(dist_max=0.6), lambda: s.fleet_ss_set_regression(off=True)),
        "per car, per row": (lambda: s.fleet_ss_set_regression(rows=ROWS, dist_max=0.6), lambda: s.fleet_ss_set_regression(off=True)),
    }
    same = lambda a, b: all(SC.bits_equal(a[k], b[k]) for k in ("X_optm", "U_optm", "status"))   # noqa: E731
    plain = _solve(s, inp)
    for name, (on, off) in regressions.items():
        on()
        regressed = _solve(s, inp)
        refused(-3, lambda: s.set_cars_controller_model(True))
        assert not s.cars_controller_model, name
        assert same(_solve(s, inp), regressed), (name, "the refused switch left the regression as it was")
        off()
        s.set_cars_controller_model(True)
        on_model = _solve(s, inp)
        refused(-3, on)
        assert s.cars_controller_model and len(s.car_vehicles()) == B, name
        assert same(_solve(s, inp), on_model), (name, "the refused regression left the model as it was")
        off()   # (switching a regression off is no error while the model is on)
        s.set_cars_controller_model(False)
    assert not SC.bits_equal(on_model["X_optm"], plain["X_optm"])
    # the two controller models: whichever is turned on second is refused, and nothing changes
    s.set_dtrack_vehicles([pkg.presets.barc_double_track()] * B)
    s.set_cars_controller_model(True)
    refused(-3, lambda: s.set_dtrack_controller_model(True))
    assert s.cars_controller_model and not s.dtrack_controller_model
    assert same(_solve(s, inp), on_model)
    s.set_cars_controller_model(False)
    s.set_dtrack_controller_model(True)
    on_dtrack = _solve(s, inp)
    refused(-3, lambda: s.set_cars_controller_model(True))
    assert s.dtrack_controller_model and not s.cars_controller_model
    assert same(_solve(s, inp), on_dtrack)
    s.set_dtrack_controller_model(False)
    s.set_dtrack_vehicles(None)
    # the sequential-QP entry while the switch is on; a batch other than the table's through every batched entry
    s.set_cars_controller_model(True)
    refused(-3, lambda: s.solve_full_dynamics(inp, max_sqp=2))
    few = {k: (v[..., :40].contiguous() if hasattr(v, "cpu") else v) for k, v in inp.items()}
    outs = SC._solve_outs(s, 40)
    outs32 = SC._solve_outs(s, 40, f32=True)
    for v in list(outs.values()) + list(outs32.values()):
        v.fill_(-3)
    refused(-1, lambda: s.solve(few, outs))
    refused(-1, lambda: s.solve(few, outs, mixed=True))
    refused(-1, lambda: s.solve(few, outs, warm=True))
    refused(-1, lambda: s.solve_f32(few, outs32))
    torch.cuda.synchronize()
    assert all(bool((v == -3).all()) for v in list(outs.values()) + list(outs32.values()))
    assert s.cars_controller_model and len(s.car_vehicles()) == B
    f32_on = s.solve_f32(inp)["X_optm"].clone()
    # freeing the table turns the switch off; with it off again a solve is the solve of a handle that never had it on
    s.set_car_vehicles(None)
    assert not s.cars_controller_model
    refused(-1, lambda: s.set_cars_controller_model(True))
    after = _solve(s, inp)
    fresh = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
    never = _solve(fresh, inp)
    for k in ("X_optm", "U_optm", "dU_optm", "status", "iters"):
        assert SC.bits_equal(after[k], plain[k]) and SC.bits_equal(after[k], never[k]), k
    assert SC.bits_equal(s.solve_f32(inp)["X_optm"], fresh.solve_f32(inp)["X_optm"]) and not SC.bits_equal(s.solve_f32(inp)["X_optm"], f32_on)
    assert (s.solve_full_dynamics(inp, max_sqp=2)["status"] == 0).float().mean() > 0.9   # and the entry that was refused runs again
    fresh.close()
    s.close()


def test_the_first_timer_times_the_new_kernel(pkg):
    """lmpc_last_kernel_ms' first number is the linearisation in front of the QP kernel, whichever kernel it is: with the switch on it
    is a positive number of milliseconds, fp64 and single precision.  (Every car on the handle's vehicle, as in the double-track
    test: a random cold start that the preset car can drive need not be one that a car with 30 % less grip can.)"""
    B = 70
    s = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
    inp = _cold(pkg, s, B, 23)
    s.set_car_vehicles([pkg.presets.barc_vehicle()] * B)
    s.set_cars_controller_model(True)
    s.enable_timing(True)
    out = _solve(s, inp)
    lin_ms, solve_ms = s.last_kernel_ms()
    assert (out["status"] == 0).all() and lin_ms > 0 and solve_ms > 0
    out = s.solve_f32(inp)
    lin_ms, solve_ms = s.last_kernel_ms()
    assert (out["status"] == 0).float().mean() > 0.9 and lin_ms > 0 and solve_ms > 0
    s.close()


def test_closed_loop_with_controllers_that_know_their_cars(pkg):
    """8 cars of three kinds, 40 periods of the tracking controller through run_lmpc_fleet_fused(plants=v, controllers=v): no failed
    solve, finite states, the switch and the table off on return, and final states other than those of the run without controllers=
    (controllers on the handle's vehicle, the same cars)."""
    B, periods = 8, 40
    tr = pkg.workloads.synthetic_track("barc")
    veh = MC.fleet(pkg.presets.barc_vehicle(), B)
    x, u = pkg.workloads.sample_initial_states("barc", B, tr["L"], [-0.01, -0.3], [0.01, 0.3], seed=17)
    x0, u0 = torch.as_tensor(x.T.copy(), device="cuda"), torch.as_tensor(u.T.copy(), device="cuda")
    mk = lambda cfg: pkg.Solver(cfg, pkg.presets.barc_vehicle(), device=0)   # noqa: E731
    runs = {}
    for name, kw in (("per-car controllers", dict(controllers=veh)), ("one controller model", {})):
        tracker, learner = mk(pkg.presets.barc_tracking_mpc(20)), mk(pkg.presets.barc_lmpc(20, 2))
        r = pkg.closed_loop.run_lmpc_fleet_fused(tracker, learner, tr, x0, u0, warm_laps=2, learn_laps=1, max_steps=periods, max_pts_per_lap=256,
                                                 plants=veh, **kw)
        assert r["steps"] == periods
        assert int(r["n_fail"].sum()) == 0, (name, r["n_fail"].cpu().numpy())
        for sv in (tracker, learner):
            assert not sv.cars_controller_model, name
            with pytest.raises(pkg.capi.LmpcError, match=r"-> -1: "):
                sv.car_vehicles()   # no table is left behind
        runs[name] = r["x"].cpu().numpy()
        if kw:   # what the argument refuses with handles in hand: nothing is left switched on
            for bad in (dict(regression={"dist_max": 0.6}), dict(plants=[dict(v) for v in veh[::-1]])):
                with pytest.raises(ValueError, match="controllers"):
                    pkg.closed_loop.run_lmpc_fleet_fused(tracker, learner, tr, x0, u0, max_steps=1, **dict(dict(plants=veh, **kw), **bad))
                assert not tracker.cars_controller_model and not learner.cars_controller_model
        tracker.close()
        learner.close()
    moved = np.abs(runs["per-car controllers"] - runs["one controller model"]).max(axis=0)
    print("final states, per-car controllers against one controller model: max |difference| per car", moved)
    assert np.isfinite(runs["per-car controllers"]).all()
    assert (moved > 1e-6).all()
