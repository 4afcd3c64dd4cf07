"""GPU: solves with the double-track controller model switched on (include/lmpc_hip_dtrack_model.h), against the DENSE optimum of the
QP built on the REFERENCE's double-track stage models (tests/dtrack_model_cases.py FIXTURES, tests/golden/dense_dtrack_*.npz: torch
restatement + autograd + oracle.qp.build_qp(lin=...), never the product's linearisation).  What this pins that the operation-level test
(tests/test_gpu_dtrack_model.py, the separate A / Bm / g arrays) cannot: the kernel's write into the solve's linearisation records,
read by the one-wave kernel (N = 20), by the two-wave kernel's own loader (N = 41, N = 40 at IAC scale) and by the learning kernel.

With the switch off the same call misses every fixture optimum by more than 1e-4: the fixtures tell the two models apart, and the
test fails without the feature.  And one closed loop: 8 four-wheel cars driven by controllers that know them."""
import numpy as np
import pytest
import torch

import dtrack_model_cases as MC
from parity import per_problem_err
from tolerances import TOL_DU, TOL_F32, TOL_XU

pytestmark = pytest.mark.gpu
GOLD = MC.__file__.rsplit("/", 1)[0] + "/golden"
KEYS = ("X_optm", "U_optm", "dU_optm")


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
            sv.set_dtrack_vehicles(table)
            ss = None if ss_x is None else (torch.as_tensor(ss_x, device="cuda"), torch.as_tensor(ss_j, device="cuda"))
            made[name] = dict(fx=fx, inp=inp, sv=sv, ss=ss, B=fx["status"].size)
        return made[name]

    yield get
    for c in made.values():
        c["sv"].close()


def solve(c, on, mixed=False, warm=None):
    sv = c["sv"]
    sv.set_dtrack_controller_model(on)
    assert sv.dtrack_controller_model == on
    if c["ss"] is None:
        return _np(sv.solve(c["inp"], mixed=mixed, warm=warm))
    o = sv.alloc_outputs(c["B"])
    o["convex_combi_optm"] = torch.zeros((c["ss"][0].shape[1], c["B"]), dtype=torch.float64, device="cuda")
    return _np(sv.solve(c["inp"], o, ss_x=c["ss"][0], ss_j=c["ss"][1], mixed=mixed, warm=warm))


@pytest.mark.parametrize("name", list(MC.FIXTURES))
def test_solve_on_the_double_track_model_against_the_dense_optimum(cases, name):
    """lmpc_solve_batch with the switch on: status 0 on every problem, X / U / dU within TOL_XU / TOL_DU (scaled) of the fixture optimum
    (for the learning set too: the weights are compared as tests/test_gpu_dense_fixtures.py compares them, through the states and
    inputs they produce).  The same call with the switch off misses the fixture by more than 1e-4 on every problem."""
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
    assert (miss > MC.MIN_DISTANCE).all(), (name, "the single-track solve is this close to the double-track optimum", miss.min(), int(np.argmin(miss)))


def test_mixed_and_warm_entries_on_the_double_track_model(cases):
    """dtrack_trk_n20 through lmpc_solve_batch_mixed (TOL_F32 against the dense optimum, tests/tolerances.py) and through
    lmpc_solve_batch_warm with the cold solution as the plan: the same answer within the contract, accepted somewhere."""
    c = cases("dtrack_trk_n20")
    sv = c["sv"]
    mixed = solve(c, True, mixed=True)
    assert sv.last_solve_precision() == "mixed"
    assert (mixed["status"] == 0).all(), np.nonzero(mixed["status"])[0]
    exu, ed = per_problem_err(mixed, c["fx"])
    print("dtrack_trk_n20 mixed: X/U max %.1e median %.1e, dU max %.1e" % (exu.max(), np.median(exu), ed.max()))
    assert exu.max() < TOL_F32 and ed.max() < TOL_F32 / 0.025, (exu.max(), ed.max())
    cold = solve(c, True)
    plan = {"X_optm_ref": torch.as_tensor(cold["X_optm"], device="cuda"), "U_optm_ref": torch.as_tensor(cold["U_optm"], device="cuda")}
    warm = solve(c, True, warm=plan)
    accepted = sv.warm_accepted(c["B"]).cpu().numpy()
    assert (warm["status"] == 0).all()
    wxu, wd = per_problem_err(warm, c["fx"])
    print("dtrack_trk_n20 warm: X/U max %.1e, dU max %.1e; accepted %d of %d, iterations mean %.2f (cold %.2f)"
          % (wxu.max(), wd.max(), accepted.sum(), accepted.size, warm["iters"].mean(), cold["iters"].mean()))
    assert wxu.max() < TOL_XU and wd.max() < TOL_DU
    assert accepted.any()
    # the warm entry with the switch off lands on the other optimum: the switch reaches this entry too
    off = solve(c, False, warm=plan)
    oxu, od = per_problem_err(off, c["fx"])
    assert (np.maximum(oxu, od) > MC.MIN_DISTANCE).all()


def test_closed_loop_with_controllers_that_know_the_car(pkg):
    """8 four-wheel cars, 40 periods of the tracking controller through run_lmpc_fleet_fused(plants_dt=v, controllers_dt=v): no
    failed solve, the switch and both tables off on return, and final states other than those of the run without controllers_dt
    (single-track controllers on the same cars)."""
    B, periods = 8, 40
    tr = pkg.workloads.synthetic_track("barc")
    veh = [MC.DT.barc_kinds(pkg.presets.barc_double_track())[b % 3] for b in range(B)]
    x, u = pkg.workloads.sample_initial_states("barc", B, tr["L"], [-0.01, -0.3], [0.01, 0.3], seed=17)
    x0, u0 = torch.as_tensor(x.T.copy(), device="cuda"), torch.as_tensor(u.T.copy(), device="cuda")
    mk = lambda cfg: pkg.Solver(cfg, pkg.presets.barc_vehicle(), device=0)   # noqa: E731
    runs = {}
    for name, kw in (("double-track controllers", dict(controllers_dt=veh)), ("single-track controllers", {})):
        tracker, learner = mk(pkg.presets.barc_tracking_mpc(20)), mk(pkg.presets.barc_lmpc(20, 2))
        r = pkg.closed_loop.run_lmpc_fleet_fused(tracker, learner, tr, x0, u0, warm_laps=2, learn_laps=1, max_steps=periods, max_pts_per_lap=256,
                                                 plants_dt=veh, **kw)
        assert r["steps"] == periods
        assert int(r["n_fail"].sum()) == 0, (name, r["n_fail"].cpu().numpy())
        for sv in (tracker, learner):
            assert not sv.dtrack_controller_model, name
            with pytest.raises(pkg.capi.LmpcError, match=r"-> -1: "):
                sv.get_dtrack_vehicles()   # no table is left behind
        runs[name] = r["x"].cpu().numpy()
        if kw:   # what the argument refuses: a regression beside it, and another list than the plant's
            for bad in (dict(regression={"dist_max": 0.6}), dict(plants_dt=[dict(v) for v in veh[::-1]])):
                with pytest.raises(ValueError, match="controllers_dt"):
                    pkg.closed_loop.run_lmpc_fleet_fused(tracker, learner, tr, x0, u0, max_steps=1, **dict(dict(plants_dt=veh, **kw), **bad))
                assert not tracker.dtrack_controller_model and not learner.dtrack_controller_model
        tracker.close()
        learner.close()
    moved = np.abs(runs["double-track controllers"] - runs["single-track controllers"]).max(axis=0)
    print("final states, double-track against single-track controllers: max |difference| per car", moved)
    assert np.isfinite(runs["double-track controllers"]).all()
    assert (moved > 1e-6).all()
