"""Every entry point that compiles the vehicle model in, on vehicles and inputs off the presets (tests/envelope_cases.py): kd inside
(0, 1) and kd = 1, Af != 1, rho != Af, every other field the dynamics read moved, u_lon saturated on both sides of the tanh blend and
at its midpoint, steer at the actuator limit, slip past the Pacejka peak.  tests/test_envelope_reference.py holds the inputs to the
audit -- every field moves the reference on them -- and the references to each other, on the CPU.

B = 130 (two waves and two lanes), N = 4 (three stages: every problem meets each band of u_lon), and B = 1 for lmpc_linearize_batch.

  lmpc_linearize_batch, lmpc_linearize_cars_batch   against the complex-step Jacobian of the oracle's integrator, PER PROBLEM: the
      error of one (problem, stage) over the largest entry of that same (problem, stage), bound envelope_cases.bounds
  lmpc_linearize_dtrack_batch                       against dtrack_model_cases.reference, measure and BOUND of test_gpu_dtrack_model
  lmpc_plant_step_batch / _cars_batch / _dtrack_batch   two sub-steps against oracle.scenario.plant_step (oracle.dynamics.rk4 behind the
      simulator's lookup and wrap) / dtrack_cases.reference, at 1e-11 max(1, |want|)
  sensitivity                                       kd, Af, rho, kb + 10 % in the table: the device leaves the envelope reference
  EKF, LQR                                          their own Jacobians of the model, through the parity paths of test_gpu_ekf / test_gpu_lqr

Needs an MI355X."""
import numpy as np
import pytest

import cars_model_cases as CM
import dtrack_cases as DT
import dtrack_model_cases as DM
import ekf_cases as EC
import envelope_cases as E
import lqr_cases as LC
import stream_cases as SC
from oracle import scenario as S

pytestmark = pytest.mark.gpu
B, N = E.B_TEST, E.N_TEST
DTRACK_BOUND = 1e-9          # tests/test_gpu_dtrack_model.py's BOUND, on |d| / max(1, |want|) element by element
PLANT_BOUND = 1e-11          # the plant tests': max |d| <= 1e-11 max(1, max |want|)
SENSITIVE = ("kd", "Af", "rho", "kb")
LQR_KEY = ("barc", 21, 0.01, 31)   # twin distance on the envelope vehicle 1.1e-15 (P0), LC.TOL_TWIN = 1e-13: qualified on the CPU


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


@pytest.fixture(scope="module")
def scene(pkg):
    solvers, cache, tracks = {}, {}, {}

    def solver(kind, integrator="rk4"):
        """a handle on the envelope vehicle"""
        if (kind, integrator) not in solvers:
            cfg = pkg.presets.barc_tracking_mpc(N) if kind == "barc" else pkg.presets.iac_tracking_mpc(N)
            solvers[kind, integrator] = pkg.Solver(cfg, dict(E.envelope_vehicle(E.base_vehicle(kind)), integrator=integrator), device=0)
        return solvers[kind, integrator]

    def track(kind):
        if kind not in tracks:
            tr = pkg.workloads.synthetic_track("barc") if kind == "barc" else DT.iac_track(pkg)
            tracks[kind] = (tr, solver(kind).device_track(tr))
        return tracks[kind]

    def lin(kind, size=B, which="single"):
        """the draws on the device, computed once"""
        if (kind, size, which) not in cache:
            inp = E.envelope_draws(kind, size, N, track=which)
            cache[kind, size, which] = dict(kind=kind, B=size, inp=inp, dev={k: dev(inp[k]) for k in E.KEYS})
        return cache[kind, size, which]

    def single(kind, veh_key, veh, size=B):
        """complex-step and analytic Jacobians of the oracle on the table `veh`, and the bounds they set, computed once"""
        d = lin(kind, size)
        if veh_key not in d:
            cs, an = E.complex_step(d["inp"], veh), CM.reference(d["inp"], veh)
            assert all(np.isfinite(a).all() for a in cs + an)
            d[veh_key] = dict(veh=veh, cs=cs, bounds=E.bounds(an, cs), spread=E.errors(an, cs))
        return d, d[veh_key]

    yield dict(solver=solver, track=track, lin=lin, single=single, pkg=pkg)
    for s in solvers.values():
        s.close()


def held(name, got, ref):
    """the device's (A, Bm, g) against the complex step per (problem, stage), printed and asserted"""
    assert all(np.isfinite(g).all() for g in got), name
    err = E.errors(got, ref["cs"])
    print("%s: worst per-problem |device - complex step|: A %.2e Bm %.2e g %.2e; the reference's own analytic-against-complex-step spread: "
          "A %.2e Bm %.2e g %.2e; worst error / bound %.2f" % (name, *(e.max() for e in err), *(s.max() for s in ref["spread"]),
                                                                max(float((e / b).max()) for e, b in zip(err, ref["bounds"]))))
    for what, e, b in zip(("A", "Bm", "g"), err, ref["bounds"]):
        assert (e <= b).all(), (name, what, float((e / b).max()), np.unravel_index(np.argmax(e / b), e.shape))


# ---- the three linearisations --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,integrator,size", [("barc", "rk4", B), ("iac", "rk4", B), ("barc", "euler", B), ("iac", "euler", B), ("barc", "rk4", 1)])
def test_linearize_batch_on_the_envelope_vehicle(scene, kind, integrator, size):
    v = dict(E.envelope_vehicle(E.base_vehicle(kind)), integrator=integrator)
    d, ref = scene["single"](kind, "handle " + integrator, [v] * size, size)
    got = [t.cpu().numpy() for t in scene["solver"](kind, integrator).linearize(d["dev"])]
    held("lmpc_linearize_batch %s %s B = %d" % (kind, integrator, size), got, ref)


@pytest.mark.parametrize("kind", E.KINDS)
def test_linearize_cars_on_the_three_car_table(scene, kind):
    d, ref = scene["single"](kind, "table", E.table(kind, B))
    s = scene["solver"](kind)
    s.set_car_vehicles(ref["veh"])
    got = [t.cpu().numpy() for t in s.linearize_cars(d["dev"])]
    held("lmpc_linearize_cars_batch %s, kd 0.35 | kd 1 | Euler by b %% 3" % kind, got, ref)
    assert len(CM.groups(ref["veh"])) == 3


@pytest.mark.parametrize("kind,integrator", [("barc", "rk4"), ("iac", "rk4"), ("barc", "euler")])
def test_a_table_of_the_handles_envelope_vehicle_is_linearize_batch_bit_for_bit(scene, kind, integrator):
    d = scene["lin"](kind)
    s = scene["solver"](kind, integrator)
    s.set_car_vehicles([dict(E.envelope_vehicle(E.base_vehicle(kind)), integrator=integrator)] * B)
    mine, theirs = s.linearize_cars(d["dev"]), s.linearize(d["dev"])
    for name, m, t in zip(("A", "Bm", "g"), mine, theirs):
        assert SC.bits_equal(m, t), (kind, integrator, name, float((m - t).abs().max()))


def dtrack_scene(scene, kind):
    d = scene["lin"](kind, B, "double")
    if "want" not in d:
        d["veh"] = E.table(kind, B, "double")
        d["want"] = DM.reference(d["inp"], d["veh"])
        assert all(np.isfinite(w).all() for w in d["want"])
    return d


def dtrack_scaled(got, want):
    return np.abs(got - want) / np.maximum(1.0, np.abs(want))


@pytest.mark.parametrize("kind", E.KINDS)
def test_linearize_dtrack_on_the_envelope_table(scene, kind):
    d = dtrack_scene(scene, kind)
    s = scene["solver"](kind)
    s.set_dtrack_vehicles(d["veh"])
    got = [t.cpu().numpy() for t in s.linearize_dtrack(d["dev"])]
    assert all(np.isfinite(g).all() for g in got)
    worst = [float(dtrack_scaled(g, w).max()) for g, w in zip(got, d["want"])]
    print("lmpc_linearize_dtrack_batch %s: max |device - reference| / max(1, |reference|): A %.3e Bm %.3e g %.3e (bound %.0e); per problem: A %.2e Bm %.2e; max |A| %.2e"
          % (kind, *worst, DTRACK_BOUND, E.per_problem(got[0], d["want"][0]).max(), E.per_problem(got[1], d["want"][1]).max(), np.abs(d["want"][0]).max()))
    assert max(worst) <= DTRACK_BOUND, worst
    assert len(DM.groups(d["veh"])) == 3


# ---- the three plant steps -----------------------------------------------------------------------------------------------------------
def plant_bound(want):
    return PLANT_BOUND * max(1.0, np.abs(want).max())


def single_plant_reference(tr, x, u, veh):
    E.check_single_plant(tr, x, u, veh)
    want = np.full((len(veh), 6), np.nan)
    for cars in CM.groups(veh):
        want[cars] = S.plant_step(CM.oracle_vehicle(veh[cars[0]]), tr, x[cars], u[cars], E.DT_SIM, E.N_SUB)
    assert np.isfinite(want).all()
    return want


@pytest.mark.parametrize("kind,integrator", [("barc", "rk4"), ("iac", "rk4"), ("barc", "euler")])
def test_plant_step_on_the_envelope_vehicle(scene, kind, integrator):
    tr, trk = scene["track"](kind)
    x, u = E.plant_draws(kind, B, tr["L"])
    want = single_plant_reference(tr, x, u, [dict(E.envelope_vehicle(E.base_vehicle(kind)), integrator=integrator)] * B)
    xs = dev(x.T)
    scene["solver"](kind, integrator).plant_step(trk, xs, dev(u.T), E.DT_SIM, E.N_SUB)
    err = np.abs(xs.cpu().numpy().T - want).max()
    print("lmpc_plant_step_batch %s %s: max |device - oracle| = %.3e, bound %.3e" % (kind, integrator, err, plant_bound(want)))
    assert err <= plant_bound(want)


@pytest.mark.parametrize("kind", E.KINDS)
def test_plant_step_cars_on_the_three_car_table(scene, kind):
    tr, trk = scene["track"](kind)
    x, u = E.plant_draws(kind, B, tr["L"])
    veh = E.table(kind, B)
    want = single_plant_reference(tr, x, u, veh)
    s = scene["solver"](kind)
    s.set_car_vehicles(veh)
    xs = dev(x.T)
    s.plant_step_cars(trk, xs, dev(u.T), E.DT_SIM, E.N_SUB)
    err = np.abs(xs.cpu().numpy().T - want).max()
    print("lmpc_plant_step_cars_batch %s: max |device - oracle| = %.3e, bound %.3e" % (kind, err, plant_bound(want)))
    assert err <= plant_bound(want)
    # the table matters: on the handle's vehicle alone the kd = 1 cars and the Euler cars miss the bound by far
    alone = single_plant_reference(tr, x, u, [veh[0]] * B)
    moved = np.abs(alone - want).max(axis=1)
    assert (moved[0::3] == 0).all() and (moved[1::3] > 1e3 * plant_bound(want)).mean() > 0.6 and (moved[2::3] > 1e3 * plant_bound(want)).all()


@pytest.mark.parametrize("kind", E.KINDS)
def test_plant_step_dtrack_on_the_envelope_table(scene, kind):
    import torch
    tr, trk = scene["track"](kind)
    x, u = E.plant_draws(kind, B, tr["L"], track="double")
    veh = E.table(kind, B, "double")
    E.check_dtrack_plant(tr, x, u, veh)
    want, gam = DT.reference(tr, x, u, veh, E.DT_SIM, E.N_SUB)
    assert np.isfinite(want).all() and np.isfinite(gam).all()
    s = scene["solver"](kind)
    s.set_dtrack_vehicles(veh)
    xs, g = dev(x.T), torch.full((B,), np.nan, dtype=torch.float64, device="cuda")
    s.plant_step_dtrack(trk, xs, dev(u.T), E.DT_SIM, E.N_SUB, g)
    err = np.abs(xs.cpu().numpy().T - want).max()
    gerr = (np.abs(g.cpu().numpy() - gam) / np.maximum(1.0, np.abs(gam))).max()
    print("lmpc_plant_step_dtrack_batch %s: max |device - reference| = %.3e, bound %.3e; gamma_y: max |device - closed form| / max(1, |gamma_y|) = %.3e, max |gamma_y| %.2e"
          % (kind, err, plant_bound(want), gerr, np.abs(gam).max()))
    assert err <= plant_bound(want)
    assert gerr <= PLANT_BOUND


# ---- the device reads kd, Af, rho and kb ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", SENSITIVE)
@pytest.mark.parametrize("kind", E.KINDS)
def test_the_device_reads_the_field(scene, kind, field):
    """A table that differs from the envelope vehicle in one field by 10 %: the device's Jacobians leave the ENVELOPE reference by
    more than 1e3 x the bound on at least a quarter of the (problem, stage) points, single track and double track."""
    env = E.envelope_vehicle(E.base_vehicle(kind))
    d, ref = scene["single"](kind, "handle rk4", [dict(env, integrator="rk4")] * B)
    s = scene["solver"](kind)
    s.set_car_vehicles([dict(env, **{field: 1.1 * env[field]})] * B)
    got = [t.cpu().numpy() for t in s.linearize_cars(d["dev"])]
    err = E.errors(got, ref["cs"])
    away = (err[0] > 1e3 * ref["bounds"][0]) | (err[1] > 1e3 * ref["bounds"][1])
    dd = dtrack_scene(scene, kind)
    if "envelope" not in dd:
        dd["envelope"] = DM.reference(dd["inp"], [dd["veh"][0]] * B)
    s.set_dtrack_vehicles([dict(dd["veh"][0], **{field: 1.1 * dd["veh"][0][field]})] * B)
    gotd = [t.cpu().numpy() for t in s.linearize_dtrack(dd["dev"])]
    awayd = np.max([dtrack_scaled(g, w).reshape(-1, N - 1, B).max(axis=0) for g, w in zip(gotd[:2], dd["envelope"][:2])], axis=0) > 1e3 * DTRACK_BOUND
    print("%s, %s + 10 %%: the device leaves the envelope reference by > 1e3 x the bound on %d (single track) and %d (double track) of %d points"
          % (kind, field, away.sum(), awayd.sum(), away.size))
    assert away.mean() >= 0.25 and awayd.mean() >= 0.25, (away.mean(), awayd.mean())


# ---- the EKF's and the LQR's own Jacobians -------------------------------------------------------------------------------------------
def ekf_scenario():
    """ekf_cases.scenario on the IAC-scale envelope vehicle: 40 periods, u_lon = 5 sin(2 pi k / 8 + phi) -- saturated on either
    side for a third of the car-periods each, and fast enough to keep vx where it started.  (A BARC-scale car leaves the filter's
    domain within a period under a saturated input: 1000 N per unit of u_lon on 2.4 kg.)  Its float64-against-longdouble twin
    distance on the CPU: x 2.0e-15, P 2.2e-16, K 3.8e-14 (ekf_cases.TOL_TWIN = 1e-13)."""
    return EC.scenario(67, periods=40, seed=5, veh=E.oracle_envelope("iac"), lon=lambda k, ph: 5.0 * np.sin(2.0 * np.pi * k / 8.0 + ph))


def test_ekf_parity_on_the_envelope_vehicle(scene):
    from test_gpu_ekf import _cmp, _scenario_filter
    sc = ekf_scenario()
    th = np.tanh(np.array([u[:, 0] for _, _, _, u, _ in sc["updates"][::2]]))
    assert (th > E.SATURATED).mean() >= 0.25 and (th < -E.SATURATED).mean() >= 0.25 and th.shape == (40, 67)
    filt, ref = _scenario_filter(scene["solver"]("iac"), sc, 67), EC.new_filter(sc)
    worst = [0.0, 0.0, 0.0]
    for obs, z, R, u, ns in sc["updates"]:
        ref.update_control(u)
        _cmp(worst, filt.update(obs, z, R, ns, u=u), ref.update(obs, z, R, ns))
    print("EKF on the IAC envelope vehicle, B = 67, %d updates: |dx| %.2e |dP| %.2e |dKz| %.2e (bound %.0e)" % (len(sc["updates"]), *worst, EC.TOL))
    assert max(worst) <= EC.TOL, worst
    scene["solver"]("iac").ekf_destroy()


def test_lqr_parity_on_the_envelope_vehicle(scene):
    from test_gpu_lqr import check, device_solve
    sc = LC.scenario(*LQR_KEY, veh=E.oracle_envelope("barc"))
    assert sc["cfg"]["N"] == 21 and sc["x_ic"].shape[0] == LC.B_TEST
    ref = LC.solve(sc["veh"], sc["cfg"], sc["x_ic"], sc["X_ref"], sc["U_ref"])
    assert not ref["flags"].any()
    check(device_solve(scene["solver"]("barc"), sc, gains=True), ref)
    scene["solver"]("barc").lqr_destroy()
