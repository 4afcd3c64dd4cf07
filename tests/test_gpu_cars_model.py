"""lmpc_linearize_cars_batch of include/lmpc_hip_cars_model.h: problem b linearised on vehicle b of the car table, against the reference
of tests/cars_model_cases.py -- the oracle's analytic Jacobian stage by stage with car b's Vehicle, never the product's own
linearisation -- on linearisation points drawn independently per stage.  B = 300 with N = 20 (a full and a partial 256-thread block,
nineteen stage rows of the grid), B = 257 with N = 3 (the smallest horizon, a tail of one lane) and B = 1.

The bound is TOL_LINEARIZE_REL (tests/tolerances.py) as tests/test_gpu_timestep.py applies it to lmpc_linearize_batch, stage by stage:
|A_i - want| <= tol max |want A_i|, the same for Bm_i, and 10 tol max(1, max |want g_i|) for g_i.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

import cars_model_cases as MC
import envelope_cases as E
import stream_cases as SC
from tolerances import TOL_LINEARIZE_REL

pytestmark = pytest.mark.gpu
KEYS = MC.KEYS
SHAPES = [(300, 20), (257, 3), (1, 20)]


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


@pytest.fixture(scope="module")
def scene(pkg):
    solvers, cache = {}, {}

    def solver(N):
        if N not in solvers:
            solvers[N] = pkg.Solver(pkg.presets.barc_tracking_mpc(N), pkg.presets.barc_vehicle(), device=0)
        return solvers[N]

    def get(B, N):
        """draws, table and the reference's answer, computed once"""
        if (B, N) not in cache:
            inp, veh = MC.lin_draws(pkg, B, N)
            want = MC.reference(inp, veh)
            assert all(np.isfinite(w).all() for w in want)
            cs = E.complex_step(inp, veh)
            assert all(np.isfinite(c).all() for c in cs)
            cache[B, N] = dict(B=B, N=N, inp=inp, veh=veh, want=want, cs=cs, dev={k: dev(inp[k]) for k in KEYS})
        return cache[B, N]

    yield dict(solver=solver, get=get, pkg=pkg)
    for s in solvers.values():
        s.close()


def linearize(scene, d, veh=None):
    s = scene["solver"](d["N"])
    s.set_car_vehicles(d["veh"] if veh is None else veh)
    return [t.cpu().numpy() for t in s.linearize_cars(d["dev"])]


def stage_errors(got, want, cs=None):
    """per stage, (error, bound) of A, Bm and g as tests/test_gpu_timestep.py scales them; with the complex-step Jacobian `cs` of the
    same table also, per array, the (problem, stage) that comes closest to its own bound in the per-problem measure of
    tests/envelope_cases.py -- a stage's largest entry belongs to its slowest car and hides an error in a fast one"""
    out = []
    if cs is not None:
        for name, e, b in zip(("A per problem", "Bm per problem", "g per problem"), E.errors(got, cs), E.bounds(want, cs)):
            j = np.unravel_index(np.argmax(e / b), e.shape)
            out.append((int(j[0]), name, float(e[j]), float(b[j])))
    for i in range(want[2].shape[1]):
        for j, tol in ((0, TOL_LINEARIZE_REL), (1, TOL_LINEARIZE_REL), (2, 10 * TOL_LINEARIZE_REL)):
            g, w = (got[j][:, :, i], want[j][:, :, i]) if j < 2 else (got[j][:, i], want[j][:, i])
            scale = float(np.abs(w).max()) if j < 2 else max(1.0, float(np.abs(w).max()))
            out.append((i, "A Bm g".split()[j], float(np.abs(g - w).max()) / scale, tol))
    return out


@pytest.mark.parametrize("B,N", SHAPES)
def test_each_problem_is_linearised_on_its_own_vehicle(scene, B, N):
    d = scene["get"](B, N)
    got = linearize(scene, d)
    assert all(np.isfinite(g).all() for g in got)
    errs = stage_errors(got, d["want"], d["cs"])
    print("B = %d N = %d, per problem against the complex step, the point closest to its bound: " % (B, N)
          + ", ".join("%s %.2e (bound %.2e)" % (m, e, t) for _, m, e, t in errs if m.endswith("per problem")))
    worst = {n: max(e for _, m, e, _ in errs if m == n) for n in ("A", "Bm", "g")}
    print("B = %d N = %d: max over stages of |device - reference| / (the stage's largest entry): A %.2e, Bm %.2e, g %.2e (bounds %.0e, %.0e, %.0e)"
          % (B, N, worst["A"], worst["Bm"], worst["g"], TOL_LINEARIZE_REL, TOL_LINEARIZE_REL, 10 * TOL_LINEARIZE_REL))
    for i, name, e, tol in errs:
        assert e <= tol, (i, name, e)
    if B >= 13:
        assert len(MC.groups(d["veh"])) == 5 and all(d["veh"][b]["integrator"] == "euler" for b in MC.EULER)


def test_the_vehicles_matter(scene, pkg):
    """Against the reference on the handle's vehicle every car's Jacobian misses by far more than the bound: all three kinds differ
    from the preset, and so do the two Euler cars from their RK4 kind."""
    d = scene["get"](300, 20)
    got = linearize(scene, d)
    preset = MC.reference(d["inp"], [pkg.presets.barc_vehicle()] * 300)
    per_car = np.abs(got[0] - preset[0]).reshape(-1, 300).max(axis=0) / np.abs(preset[0]).max()
    assert (per_car > 1e3 * TOL_LINEARIZE_REL).all(), per_car.min()
    rk4 = linearize(scene, d, veh=[dict(v, integrator="rk4") for v in d["veh"]])
    diff = np.abs(got[0] - rk4[0]).reshape(-1, 300).max(axis=0)
    euler = np.isin(np.arange(300), MC.EULER)
    assert (diff[~euler] == 0).all() and (diff[euler] > 1e3 * TOL_LINEARIZE_REL).all()


@pytest.mark.parametrize("B,N", SHAPES)
def test_a_table_of_the_handles_vehicle_agrees_with_linearize_batch(scene, pkg, B, N):
    """Every car on the handle's vehicle: the two kernels share the model text and must agree within the tolerance each is held to;
    whether they agree to the last bit is reported, not asserted."""
    d = scene["get"](B, N)
    mine = linearize(scene, d, veh=[pkg.presets.barc_vehicle()] * B)
    theirs = [t.cpu().numpy() for t in scene["solver"](N).linearize(d["dev"])]
    errs = stage_errors(mine, theirs)
    print("B = %d N = %d, every car on the handle's vehicle: lmpc_linearize_cars_batch against lmpc_linearize_batch: worst relative difference %.2e; "
          "bit-equal: %s" % (B, N, max(e for _, _, e, _ in errs), all(np.array_equal(m, t) for m, t in zip(mine, theirs))))
    for i, name, e, tol in errs:
        assert e <= tol, (i, name, e)


def test_refusals_leave_the_outputs_untouched(scene, pkg):
    import torch
    d = scene["get"](257, 3)
    B = 257
    s = pkg.Solver(pkg.presets.barc_tracking_mpc(3), pkg.presets.barc_vehicle(), device=0)
    out = tuple(torch.full(sh, -3.0, dtype=torch.float64, device="cuda") for sh in ((6, 6, 2, B), (6, 2, 2, B), (6, 2, B)))

    def refused(code, call):
        with pytest.raises(pkg.capi.LmpcError, match=r"-> %d: " % code):
            call()

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == -3.0).all()) for t in out)

    # no table: the linearisation and the switch
    refused(-1, lambda: s.linearize_cars(d["dev"], out=out))
    refused(-1, lambda: s.set_cars_controller_model(True))
    assert untouched() and not s.cars_controller_model
    s.set_cars_controller_model(False)   # off without a table is no error
    # a table of 40: another batch
    s.set_car_vehicles(d["veh"][:40])
    refused(-1, lambda: s.linearize_cars(d["dev"], out=out))
    assert untouched() and len(s.car_vehicles()) == 40
    # NULL pointers, one at a time
    s.set_car_vehicles(d["veh"])
    ptrs = [d["dev"][k].data_ptr() for k in KEYS] + [t.data_ptr() for t in out]
    for j in range(7):
        a = [C.c_void_p(None if i == j else p) for i, p in enumerate(ptrs)]
        assert s.lib.lmpc_linearize_cars_batch(s._h, C.c_int32(B), *a) == -1, j
    assert s.lib.lmpc_cars_get_controller_model(s._h, None) == -1
    assert untouched()
    # and the call that is not refused writes every element, with the switch off as with it on
    off = [t.clone() for t in s.linearize_cars(d["dev"], out=out)]
    assert all(bool((t != -3.0).all()) for t in off)
    s.set_cars_controller_model(True)
    on = s.linearize_cars(d["dev"])
    assert all(SC.bits_equal(a, b) for a, b in zip(on, off))
    s.close()
