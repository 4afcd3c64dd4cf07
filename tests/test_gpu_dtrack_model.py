"""lmpc_linearize_dtrack_batch and the switch of include/lmpc_hip_dtrack_model.h: problem b linearised on the four-wheel model by
vehicle b of the double-track table, against the reference of tests/dtrack_model_cases.py -- the torch restatement of
tests/dtrack_cases.py with the closed-form gamma_y, Jacobians by autograd, once per distinct vehicle.  B = 70 with N = 3 and B = 300
with N = 20: a full and a partial wave, a full and a partial 256-thread block, two and nineteen stage rows of the grid.

The bound, element-wise on A, Bm and g: 1e-9 max(1, |want|) -- the bound the project holds the double-track rollouts to, for the same
reason: the kernel iterates gamma_y by Newton where the reference takes the closed form (and differentiates the iterate by the
implicit-function theorem where the reference differentiates the root).  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

import dtrack_cases as DT
import dtrack_model_cases as MC
import stream_cases as SC

pytestmark = pytest.mark.gpu
BOUND = 1e-9
KEYS = ("X_ref", "U_ref", "T_ref", "curvatures")
S345 = (3, 4, 5)
ROWS = {3: (S345, (0,)), 4: (S345, (1,)), 5: (S345, (1,))}


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


@pytest.fixture(scope="module")
def scene(pkg):
    solvers, cache = {}, {}

    def solver(kind, N):
        if (kind, N) not in solvers:
            cfg, veh = ((pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle()) if kind == "barc" else
                        (pkg.presets.iac_tracking_mpc(N), pkg.presets.iac_vehicle()))
            solvers[kind, N] = pkg.Solver(cfg, veh, device=0)
        return solvers[kind, N]

    def get(kind, B, N):
        """draws, table and the reference's answer, computed once"""
        if (kind, B, N) not in cache:
            inp, veh = MC.lin_draws(pkg, kind, B, N)
            want = MC.reference(inp, veh)
            known = np.ones((N - 1, B), dtype=bool)   # the knot under the speed guard is held to `finite`, not to the reference
            if kind == "barc":
                known[MC.SLOW[1], MC.SLOW[0]] = False
            assert all(np.isfinite(w[..., known]).all() for w in want)
            cache[kind, B, N] = dict(kind=kind, B=B, N=N, inp=inp, veh=veh, want=want, known=known, dev={k: dev(inp[k]) for k in KEYS})
        return cache[kind, B, N]

    yield dict(solver=solver, get=get, pkg=pkg)
    for s in solvers.values():
        s.close()


def linearize(scene, d, order=None, veh=None):
    import torch
    s = scene["solver"](d["kind"], d["N"])
    veh = d["veh"] if veh is None else veh
    inp = d["dev"]
    if order is not None:
        at = torch.as_tensor(order, device="cuda")
        veh, inp = [veh[b] for b in order], {k: v[..., at].contiguous() for k, v in inp.items()}
    s.set_dtrack_vehicles(veh)
    return s.linearize_dtrack(inp)


def scaled(got, want):
    return np.abs(got - want) / np.maximum(1.0, np.abs(want))


@pytest.mark.parametrize("kind,B,N", [("barc", 70, 3), ("barc", 300, 20), ("iac", 70, 3), ("iac", 300, 20)])
def test_each_problem_is_linearised_on_the_double_track_model_of_its_own_vehicle(scene, kind, B, N):
    d = scene["get"](kind, B, N)
    got = [t.cpu().numpy() for t in linearize(scene, d)]
    worst = {}
    for name, g, w in zip(("A", "Bm", "g"), got, d["want"]):
        assert np.isfinite(g).all(), name
        e = scaled(g, w)[..., d["known"]]
        worst[name] = float(e.max())
    print("%s B = %d N = %d: max |device - reference| / max(1, |reference|): A %.3e, Bm %.3e, g %.3e (bound %.0e); max |A| %.2e, |Bm| %.2e"
          % (kind, B, N, worst["A"], worst["Bm"], worst["g"], BOUND, np.abs(d["want"][0][..., d["known"]]).max(),
             np.abs(d["want"][1][..., d["known"]]).max()))
    assert max(worst.values()) <= BOUND, worst
    if kind == "barc":
        assert len(MC.groups(d["veh"])) == 5 and all(d["veh"][b]["integrator"] == "euler" for b in MC.EULER)


def test_the_knot_under_the_speed_guard_gives_finite_outputs(scene):
    d = scene["get"]("barc", 70, 3)
    b, i = MC.SLOW
    assert np.hypot(d["inp"]["X_ref"][3, i, b], d["inp"]["X_ref"][4, i, b]) < 1e-6 and d["inp"]["X_ref"][3, i, b] == 3e-7
    A, Bm, g = (t.cpu().numpy() for t in linearize(scene, d))
    assert np.isfinite(A[:, :, i, b]).all() and np.isfinite(Bm[:, :, i, b]).all() and np.isfinite(g[:, i, b]).all()
    assert np.array_equal(A[:, 0, i, b], np.eye(6)[0])   # nothing reads s


@pytest.mark.parametrize("B,N", [(70, 3), (300, 20)])
def test_permuting_problems_and_table_permutes_the_result_bit_for_bit(scene, B, N):
    import torch
    d = scene["get"]("barc", B, N)
    straight = linearize(scene, d)
    order = np.random.default_rng(5).permutation(B)
    assert (order != np.arange(B)).sum() > B // 2
    permuted = linearize(scene, d, order=order)
    at = torch.as_tensor(order, device="cuda")
    for p, s in zip(permuted, straight):
        assert SC.bits_equal(p, s[..., at].contiguous())


def test_the_vehicles_matter(scene, pkg):
    """Against a table of the preset alone: the RK4 cars of the preset get the same bits, every car of the two other kinds (and the
    two Euler cars) differs by more than 100 x the bound."""
    d = scene["get"]("barc", 300, 20)
    mine = [t.cpu().numpy() for t in linearize(scene, d)]
    preset = [t.cpu().numpy() for t in linearize(scene, d, veh=[pkg.presets.barc_double_track()] * 300)]
    per_car = np.max([scaled(m, p).reshape(-1, 300).max(axis=0) for m, p in zip(mine, preset)], axis=0)
    kind = np.arange(300) % 3
    euler = np.isin(np.arange(300), MC.EULER)
    assert (per_car[(kind == 0) & ~euler] == 0).all()
    assert (per_car[(kind != 0) | euler] > 100 * BOUND).all(), per_car[(kind != 0) | euler].min()


def cold(pkg, s, B, seed):
    tr = pkg.workloads.synthetic_track("barc")
    trk = s.device_track(tr)
    L = float(tr["L"])
    return dict(SC._cold_inputs(pkg, s, trk, L, seed, n=B), L=L), trk


def solve(s, inp, **kw):
    out = s.solve(inp, SC._solve_outs(s, inp["x_ic"].shape[1]), **kw)
    return {k: v for k, v in out.items() if hasattr(v, "cpu")}


def test_the_workspace_form_through_a_solve(scene, pkg):
    """The records the QP kernels read are written per (problem, stage): with the switch on, permuting problems and table permutes the
    solutions bit for bit; and with every car on ONE vehicle of the table, the cars that had that vehicle in the mixed table get the
    bits they got there -- a car's record comes from its own row of the table and from nothing else."""
    import torch
    B = 70
    s = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
    inp, _ = cold(pkg, s, B, 21)
    veh = [DT.barc_kinds(pkg.presets.barc_double_track())[b % 3] for b in range(B)]
    s.set_dtrack_vehicles(veh)
    s.set_dtrack_controller_model(True)
    straight = solve(s, inp)
    assert (straight["status"] == 0).all()
    order = np.random.default_rng(6).permutation(B)
    at = torch.as_tensor(order, device="cuda")
    s.set_dtrack_vehicles([veh[b] for b in order])
    assert s.dtrack_controller_model, "replacing the table keeps the switch on"
    permuted = solve(s, {k: (v[..., at].contiguous() if hasattr(v, "cpu") else v) for k, v in inp.items()})
    for k in ("X_optm", "U_optm", "dU_optm", "status", "iters"):
        assert SC.bits_equal(permuted[k], straight[k][..., at].contiguous()), k
    s.set_dtrack_vehicles([veh[2]] * B)
    one = solve(s, inp)
    cars = torch.arange(2, B, 3, device="cuda")
    others = torch.arange(1, B, 3, device="cuda")
    for k in ("X_optm", "U_optm", "dU_optm"):
        assert SC.bits_equal(one[k][..., cars].contiguous(), straight[k][..., cars].contiguous()), k
    assert not (one["X_optm"][..., others] == straight["X_optm"][..., others]).all(dim=(0, 1)).any()
    s.close()


def test_refusals_leave_outputs_table_and_switch_untouched(scene, pkg):
    import torch
    d = scene["get"]("barc", 70, 3)
    s = pkg.Solver(pkg.presets.barc_tracking_mpc(3), pkg.presets.barc_vehicle(), device=0)
    fill = lambda: tuple(torch.full(sh, -3.0, dtype=torch.float64, device="cuda") for sh in ((6, 6, 2, 70), (6, 2, 2, 70), (6, 2, 70)))   # noqa: E731

    def refused(code, call):
        with pytest.raises(pkg.capi.LmpcError, match=r"-> %d: " % code):
            call()

    def untouched(out):
        torch.cuda.synchronize()
        return all(bool((t == -3.0).all()) for t in out)

    # no table: the linearisation and the switch
    out = fill()
    refused(-1, lambda: s.linearize_dtrack(d["dev"], out=out))
    refused(-1, lambda: s.set_dtrack_controller_model(True))
    assert untouched(out) and not s.dtrack_controller_model
    s.set_dtrack_controller_model(False)   # off without a table is no error
    # a table of 40: another batch
    s.set_dtrack_vehicles(d["veh"][:40])
    refused(-1, lambda: s.linearize_dtrack(d["dev"], out=out))
    assert untouched(out) and len(s.get_dtrack_vehicles()) == 40
    # NULL pointers, one at a time
    s.set_dtrack_vehicles(d["veh"])
    ptrs = [d["dev"][k].data_ptr() for k in KEYS] + [t.data_ptr() for t in out]
    for j in range(7):
        a = [C.c_void_p(None if i == j else p) for i, p in enumerate(ptrs)]
        assert s.lib.lmpc_linearize_dtrack_batch(s._h, C.c_int32(70), *a) == -1, j
    assert s.lib.lmpc_dtrack_get_controller_model(s._h, None) == -1
    assert untouched(out)
    want = s.linearize_dtrack(d["dev"])
    s.close()

    # the switch against each regression, in both orders; the f32 and SQP entries while it is on
    B = 70
    s = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
    inp, _ = cold(pkg, s, B, 22)
    veh = [DT.barc_kinds(pkg.presets.barc_double_track())[b % 3] for b in range(B)]
    s.set_dtrack_vehicles(veh)
    x, u = pkg.workloads.sample_initial_states("barc", 6, inp["L"], [-0.01, -0.3], [0.01, 0.3], seed=9)
    laps = [(x, u, np.zeros(6), 0.03 * np.arange(6))]
    s.fleet_ss_create(B, 64)
    regressions = {
        "shared": (lambda: s.set_regression_laps(laps, dist_max=0.6), lambda: s.set_regression_laps([])),
        "shared, per row": (lambda: s.set_regression_laps(laps, rows=ROWS, dist_max=0.6), lambda: s.set_regression_laps([])),
        "per car": (lambda: s.fleet_ss_set_regression(dist_max=0.6), lambda: s.fleet_ss_set_regression(off=True)),
        "per car, per row": (lambda: s.fleet_ss_set_regression(rows=ROWS, dist_max=0.6), lambda: s.fleet_ss_set_regression(off=True)),
    }
    plain = solve(s, inp)
    for name, (on, off) in regressions.items():
        on()
        regressed = solve(s, inp)
        refused(-3, lambda: s.set_dtrack_controller_model(True))
        assert not s.dtrack_controller_model, name
        again = solve(s, inp)
        assert all(SC.bits_equal(again[k], regressed[k]) for k in ("X_optm", "U_optm", "status")), (name, "the refused switch left the regression as it was")
        off()
        s.set_dtrack_controller_model(True)
        on_model = solve(s, inp)
        refused(-3, on)
        assert s.dtrack_controller_model, name
        assert len(s.get_dtrack_vehicles()) == B
        again = solve(s, inp)
        assert all(SC.bits_equal(again[k], on_model[k]) for k in ("X_optm", "U_optm", "status")), (name, "the refused regression left the model as it was")
        off()   # (switching a regression off is no error while the model is on)
        s.set_dtrack_controller_model(False)
    # f32 and the sequential-QP entry while the switch is on; a batch other than the table's
    s.set_dtrack_controller_model(True)
    refused(-3, lambda: s.solve_f32(inp))
    refused(-3, lambda: s.solve_full_dynamics(inp, max_sqp=2))
    few = {k: (v[..., :40].contiguous() if hasattr(v, "cpu") else v) for k, v in inp.items()}
    outs = SC._solve_outs(s, 40)
    for v in outs.values():
        v.fill_(-3)
    refused(-1, lambda: s.solve(few, outs))
    refused(-1, lambda: s.solve(few, outs, mixed=True))
    refused(-1, lambda: s.solve(few, outs, warm=True))
    torch.cuda.synchronize()
    assert all(bool((v == -3).all()) for v in outs.values())
    assert s.dtrack_controller_model and len(s.get_dtrack_vehicles()) == B
    # freeing the table turns the switch off; with it off again a solve is the solve of a handle that never had it on
    s.set_dtrack_vehicles(None)
    assert not s.dtrack_controller_model
    after = solve(s, inp)
    for k in ("X_optm", "U_optm", "dU_optm", "status", "iters"):
        assert SC.bits_equal(after[k], plain[k]), k
    fresh = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
    never = solve(fresh, inp)
    for k in ("X_optm", "U_optm", "dU_optm", "status", "iters"):
        assert SC.bits_equal(after[k], never[k]), k
    assert not SC.bits_equal(on_model["X_optm"], plain["X_optm"])
    assert (s.solve_f32(inp)["status"] == 0).float().mean() > 0.9   # and the entries that were refused run again
    fresh.close()
    s.close()
    assert all(torch.isfinite(t).all() for t in want)


def test_the_first_timer_times_the_new_kernel(pkg):
    """lmpc_last_kernel_ms' first number is the linearisation in front of the QP kernel, whichever model it is on: with the switch
    on it is a positive number of milliseconds, and the solve behind it is the one the switch selects."""
    B = 70
    s = pkg.Solver(pkg.presets.barc_tracking_mpc(20), pkg.presets.barc_vehicle(), device=0)
    inp, _ = cold(pkg, s, B, 23)
    s.set_dtrack_vehicles([pkg.presets.barc_double_track()] * B)
    s.set_dtrack_controller_model(True)
    s.enable_timing(True)
    out = solve(s, inp)
    lin_ms, solve_ms = s.last_kernel_ms()
    assert (out["status"] == 0).all() and lin_ms > 0 and solve_ms > 0
    s.close()
