"""closed_loop.run_lmpc_fleet(..., plants_dt=...): single-track controllers driving four-wheel cars, the double-track plant of
include/lmpc_hip_dtrack.h in the fleet experiment's `plant` hook.  8 cars, 60 periods, tracking only (no car closes a lap in 60
periods, so the learning controller never starts).  What is claimed: the run is finite, every car advances, the run clears the
table it set, and the cars end elsewhere than on the single-track plant.  Whether the cars stay inside the boundaries under this
plant is NOT claimed; what was seen is in profiles/dtrack_plant.md.  Needs an MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, PERIODS = 8, 60


def test_sixty_periods_on_four_wheel_cars(pkg):
    import torch
    tr = pkg.workloads.synthetic_track("barc")
    rng = np.random.default_rng(0)
    x0 = np.stack([np.full(B, 0.5), rng.uniform(-0.05, 0.05, B), np.zeros(B), np.full(B, 2.0), np.zeros(B), np.zeros(B)])
    x0 = torch.as_tensor(x0, device="cuda")
    u0 = torch.zeros((2, B), dtype=torch.float64, device="cuda")
    base = pkg.presets.barc_double_track()
    kinds = (base, dict(base, mu=0.7), dict(base, kroll_f=0.35, Ef=0.6, Er=0.6))
    plants_dt = [kinds[b % 3] for b in range(B)]
    res = {}
    for key, kw in (("double", dict(plants_dt=plants_dt)), ("single", {})):
        tracker = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
        learner = pkg.Solver(pkg.presets.barc_lmpc(20, 3), pkg.presets.barc_vehicle(), device=0)
        res[key] = pkg.closed_loop.run_lmpc_fleet(tracker, learner, tr, x0, u0, max_steps=PERIODS, **kw)
        torch.cuda.synchronize()
        if kw:
            with pytest.raises(pkg.LmpcError):       # the run cleared the table it set
                learner.get_dtrack_vehicles()
            single = [pkg.presets.barc_vehicle()] * B
            with pytest.raises(ValueError):
                pkg.closed_loop.run_lmpc_fleet(tracker, learner, tr, x0, u0, max_steps=1, plants_dt=plants_dt, plants=single)
            with pytest.raises(ValueError):
                pkg.closed_loop.run_lmpc_fleet(tracker, learner, tr, x0, u0, max_steps=1, plants_dt=plants_dt, plant=tracker)
            with pytest.raises(ValueError):
                pkg.closed_loop.run_lmpc_fleet(tracker, learner, tr, x0, u0, max_steps=1, plants_dt=plants_dt[:-1])
        tracker.close(), learner.close()
    a, b = res["double"], res["single"]
    assert a["steps"] == b["steps"] == PERIODS
    xa, xb = a["x"].cpu().numpy(), b["x"].cpu().numpy()
    assert np.isfinite(xa).all()
    assert all(k == [] for k in a["lap_kind"])                      # tracking only: no lap closed, no car learnt
    advanced = xa[0] - x0[0].cpu().numpy()
    print("four-wheel plant, %d periods: advance %.2f .. %.2f m (single-track plant %.2f .. %.2f), worst boundary excess %.3f m (%.3f), "
          "failed solves %d (%d), max |final state - single-track run| per car %s"
          % (PERIODS, advanced.min(), advanced.max(), (xb[0] - 0.5).min(), (xb[0] - 0.5).max(), float(a["worst_excess"].max()),
             float(b["worst_excess"].max()), int(a["n_fail"].sum()), int(b["n_fail"].sum()), np.abs(xa - xb).max(axis=0).round(4)))
    assert (advanced > 0).all()
    assert (np.abs(xa - xb).max(axis=0) > 1e-6).all()
