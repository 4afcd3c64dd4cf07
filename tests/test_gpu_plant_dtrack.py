"""The double-track table of include/lmpc_hip_dtrack.h and lmpc_plant_step_dtrack_batch: car b stepped on the four-wheel model by
vehicle b, against the plain restatement of tests/dtrack_cases.py (which takes gamma_y from the closed-form root where the kernel
iterates) run once per distinct vehicle on that vehicle's cars.  B = 70 and B = 300: a full and a partial wave, a full and a partial
256-thread block.  The bound is the one lmpc_plant_step_batch and lmpc_plant_step_cars_batch are held to.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

import dtrack_cases as DC

pytestmark = pytest.mark.gpu

DT_SIM, N_SUB, SLOW, LINE, EULER = DC.DT_SIM, DC.N_SUB, DC.SLOW, DC.LINE, DC.EULER


@pytest.fixture(scope="module")
def scene(pkg):
    solver = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
    tracks = {"barc": pkg.workloads.synthetic_track("barc"), "iac": DC.iac_track(pkg)}
    trks = {k: solver.device_track(t) for k, t in tracks.items()}
    cache = {}

    def get(name, B):
        """draws, table and the reference's answer, computed once"""
        if (name, B) not in cache:
            tr = tracks[name]
            if name == "barc":
                x, u, veh = DC.barc_draws(pkg, B, tr["L"])
            else:
                x, u = DC.iac_draws(B, tr["L"])
                veh = [pkg.presets.iac_double_track()] * B
            want, gam = DC.reference(tr, x, u, veh)
            assert np.isfinite(want).all() and np.isfinite(gam).all()
            cache[name, B] = dict(name=name, x=x, u=u, veh=veh, want=want, gam=gam, tr=tr, trk=trks[name])
        return cache[name, B]

    yield dict(solver=solver, get=get, pkg=pkg)
    solver.close()


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def step(scene, d, order=None, n_sub=N_SUB, launches=1, gamma=True, x=None, u=None, trk=None):
    import torch
    order = np.arange(len(d["veh"])) if order is None else order
    scene["solver"].set_dtrack_vehicles([d["veh"][b] for b in order])
    xs, ua = dev((d["x"] if x is None else x)[order].T), dev((d["u"] if u is None else u)[order].T)
    g = torch.full((len(order),), np.nan, dtype=torch.float64, device="cuda") if gamma else None
    for _ in range(launches):
        scene["solver"].plant_step_dtrack(d["trk"] if trk is None else trk, xs, ua, DT_SIM, n_sub, g)
    return xs, g


def bound(want):
    return 1e-11 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("name,B", [("barc", 70), ("barc", 300), ("iac", 70), ("iac", 300)])
def test_each_car_is_stepped_on_the_double_track_model_by_its_own_vehicle(scene, name, B):
    d = scene["get"](name, B)
    xs, g = step(scene, d)
    got, gam = xs.cpu().numpy().T, g.cpu().numpy()
    want = d["want"]
    err = np.abs(got - want).max()
    gerr = (np.abs(gam - d["gam"]) / np.maximum(1.0, np.abs(d["gam"]))).max()
    print("%s B = %d: max |device - reference| = %.3e, bound %.3e; gamma_y: max |device - closed form| / max(1, |gamma_y|) = %.3e, "
          "max |gamma_y| = %.3e" % (name, B, err, bound(want), gerr, np.abs(d["gam"]).max()))
    assert err <= bound(want)
    assert (np.abs(gam - d["gam"]) <= 1e-11 * np.maximum(1.0, np.abs(d["gam"]))).all()
    L = d["tr"]["L"]
    assert (got[:, 0] >= 0).all() and (got[:, 0] < L).all()
    if name == "barc":
        assert got[LINE, 0] < 0.1 * L and d["x"][LINE, 0] > 0.9 * L   # that car did cross the line
        assert np.hypot(d["x"][SLOW, 3], d["x"][SLOW, 4]) < 1e-6      # and that one is under the guard
        # the cases are what they are meant to be: vehicle and integrator matter far beyond the bound (the grip on every car of
        # its kind; roll share and falloff where a car slips, which nine in ten of the draws do by more than 1e-6)
        preset = [scene["pkg"].presets.barc_double_track()] * B
        moved = np.abs(DC.reference(d["tr"], d["x"], d["u"], preset)[0] - want).max(axis=1)
        third = np.array([b for b in range(2, B, 3) if b != SLOW])   # (the guard car has no lateral motion at all)
        assert (moved[1::3] > 1e-6).all() and (moved[third] > 1e-6).mean() > 0.9 and (moved[list(EULER)] > 1e-6).all()
        assert (moved[third] > 100 * bound(want)).all()
        assert len({tuple(sorted(v.items())) for v in d["veh"]}) == 5
    else:
        assert np.abs(d["gam"]).max() > 1e3   # the scale at which the Newton count matters


@pytest.mark.parametrize("name", ["barc", "iac"])
def test_mirror_symmetry_on_the_device(scene, name):
    """e_y, e_psi, vy, omega, STEER and the curvature negated: exactly those outputs negated, within the bound of the step itself."""
    d = scene["get"](name, 300)
    straight, g = step(scene, d)
    mtrk = scene["solver"].device_track(dict(d["tr"], curvature=-d["tr"]["curvature"]))
    mirrored, gm = step(scene, d, x=d["x"] * DC.MIRROR_X, u=d["u"] * DC.MIRROR_U, trk=mtrk)
    a, b = straight.cpu().numpy().T, mirrored.cpu().numpy().T * DC.MIRROR_X
    print("%s: max |mirror(step(mirror)) - step| = %.3e" % (name, np.abs(a - b).max()))
    assert np.abs(a - b).max() <= bound(d["want"])
    assert (np.abs(g.cpu().numpy() + gm.cpu().numpy()) <= 1e-11 * np.maximum(1.0, np.abs(d["gam"]))).all()


@pytest.mark.parametrize("B", [70, 300])
def test_permuting_cars_and_table_permutes_the_result(scene, B):
    import torch
    d = scene["get"]("barc", B)
    straight, g = step(scene, d)
    order = np.random.default_rng(3).permutation(B)
    assert (order != np.arange(B)).sum() > B // 2
    permuted, gp = step(scene, d, order=order)
    at = torch.as_tensor(order, device="cuda")
    assert torch.equal(permuted, straight[:, at]) and torch.equal(gp, g[at])


@pytest.mark.parametrize("name,B", [("barc", 70), ("barc", 300), ("iac", 300)])
def test_two_launches_of_one_sub_step_are_one_of_two(scene, name, B):
    """They differ by the conversion to (vx, vy) and back between the two sub-steps only: the bound of the step itself."""
    d = scene["get"](name, B)
    two, g2 = step(scene, d, n_sub=1, launches=2)
    one, g1 = step(scene, d, n_sub=2)
    err = np.abs(two.cpu().numpy() - one.cpu().numpy()).max()
    print("%s B = %d: max |two launches - one| = %.3e" % (name, B, err))
    assert err <= bound(d["want"])
    assert (np.abs(g2.cpu().numpy() - g1.cpu().numpy()) <= 1e-11 * np.maximum(1.0, np.abs(d["gam"]))).all()


@pytest.mark.parametrize("B", [70, 300])
def test_without_the_gamma_output_the_state_is_the_same_to_the_bit(scene, B):
    import torch
    d = scene["get"]("barc", B)
    assert torch.equal(step(scene, d, gamma=False)[0], step(scene, d)[0])


def test_the_table_reads_back_as_it_was_set(scene):
    d = scene["get"]("barc", 70)
    scene["solver"].set_dtrack_vehicles(d["veh"])
    back = scene["solver"].get_dtrack_vehicles()
    assert len(back) == 70
    for b, (got, want) in enumerate(zip(back, d["veh"])):
        want = dict(want, integrator={"rk4": 0, "euler": 1}[want["integrator"]])
        assert got == want, b


def test_refusals_leave_the_state_and_the_table_as_they_were(scene, pkg):
    import torch
    d, s = scene["get"]("barc", 70), scene["solver"]
    trk = d["trk"]
    x0, ua = dev(d["x"].T), dev(d["u"].T)
    g0 = torch.full((70,), -3.0, dtype=torch.float64, device="cuda")

    def refused(call):
        with pytest.raises(pkg.capi.LmpcError, match=r"-> -1: "):   # LMPC_ERR_ARGUMENT
            call()

    # no table (and the single-track car table does not stand in for it)
    s.set_dtrack_vehicles(None)
    s.set_car_vehicles([pkg.presets.barc_vehicle()] * 70)
    xs, g = x0.clone(), g0.clone()
    refused(lambda: s.plant_step_dtrack(trk, xs, ua, DT_SIM, N_SUB, g))
    refused(lambda: s.get_dtrack_vehicles())
    s.set_car_vehicles(None)
    assert torch.equal(xs, x0) and torch.equal(g, g0)
    # a table of 70: another batch
    want = step(scene, d)[0]
    x300, u300 = dev(np.tile(d["x"], (5, 1))[:300].T), dev(np.tile(d["u"], (5, 1))[:300].T)
    keep = x300.clone()
    refused(lambda: s.plant_step_dtrack(trk, x300, u300, DT_SIM, N_SUB))
    assert torch.equal(x300, keep)
    # a vehicle that is refused, or a negative batch: the table in force stays in force
    for bad in (dict(model_id=0), dict(integrator=7), dict(tw_f=-0.3, tw_r=0.3), dict(Fz0_f=0.0), dict(Fz0_r=0.0)):
        veh = list(d["veh"])
        veh[33] = dict(veh[33], **bad)
        refused(lambda: s.set_dtrack_vehicles(veh))
        refused(lambda: s.set_dtrack_vehicles(veh[:40]))
        xs = x0.clone()
        s.plant_step_dtrack(trk, xs, ua, DT_SIM, N_SUB)
        assert torch.equal(xs, want)
        assert len(s.get_dtrack_vehicles()) == 70
    arr = (pkg.capi.CVehicleDT * 1)()
    assert s.lib.lmpc_dtrack_set_vehicles(s._h, C.c_int32(-1), arr) == -1
    assert len(s.get_dtrack_vehicles()) == 70
    # NULL track, NULL state, NULL input, a bad track, dt_sim not positive, n_sub < 1
    xs, g = x0.clone(), g0.clone()
    ct = s._ctrack(trk)
    bad_ct = s._ctrack(trk)
    bad_ct.M = 0
    ok = dict(track=C.byref(ct), x=xs.data_ptr(), u=ua.data_ptr(), dt=DT_SIM, n=N_SUB)
    for change in (dict(track=None), dict(x=None), dict(u=None), dict(track=C.byref(bad_ct)), dict(dt=0.0), dict(dt=-DT_SIM), dict(n=0)):
        a = dict(ok, **change)
        rc = s.lib.lmpc_plant_step_dtrack_batch(s._h, C.c_int32(70), a["track"], C.c_void_p(a["x"]), C.c_void_p(a["u"]), C.c_double(a["dt"]),
                                                C.c_int32(a["n"]), C.c_void_p(g.data_ptr()))
        assert rc == -1, change
    torch.cuda.synchronize()
    assert torch.equal(xs, x0) and torch.equal(g, g0)
    s.plant_step_dtrack(trk, xs, ua, DT_SIM, N_SUB)
    assert torch.equal(xs, want)
    # lmpc_create does not build the model as a controller's: only the plant exists
    with pytest.raises(pkg.capi.LmpcError):
        pkg.Solver(pkg.presets.barc_tracking_mpc(20), dict(pkg.presets.barc_vehicle(), model_id=2), device=0)
