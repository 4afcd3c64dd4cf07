"""GPU: the two-wavefronts-per-problem kernels (csrc/lmpc_solve_w2.hip.h) through exits of the interior point that skip the
active-set polish.  Both waves of a problem run one body, lmpc_solve_problem (csrc/lmpc_solve_kernel.hip), each on its half of the
slots; every scalar a branch depends on is agreed between them through LDS.  tests/test_gpu_two_waves.py and
tests/test_gpu_two_wave_polish.py hold those kernels on the converged path; the places where the two waves could still disagree on a
branch -- one leaves the iteration, the other waits at a barrier for good, or the answers differ -- are the other ways out:
  * x_ic outside the state box at knot 0: no iteration at all (a quarter of the problems start with vx above its upper bound);
  * the iteration cap, `it == max_iter` (lmpc_config.max_iter = 3).
Shapes: 64 problems of the BARC tracking preset at N = 24, 41 and 65, one horizon per slot class (KQ = 7 / 11 / 14: 4 / 6 / 7 slots
per lane; the first forced with set_waves_per_problem(2)).  Each case solves with two waves per problem and then with one on the same
inputs and compares as tests/test_gpu_two_waves.py compares the two kernels: statuses and iteration counts equal on every problem,
X / U / dU to 1e-8 (scaled) on every problem whose status is the same in both and not INFEASIBLE.  (MI355X: the two kernels agree to
3e-12 in X, 4e-12 in U and 4e-11 in dU in every case.)
Not here: the polish switched off (lmpc_config.polish = -1).  Held to the same rule it does not pass, before or after the two kernels
shared their body: with no polish to verify the interior point's own answer, the two kernels -- whose sweeps differ in the last
bits -- disagree on the status and the iteration count of one problem of the 64 at N = 41 and at N = 65 (a stall that only one of them
calls moving), and their unpolished iterates are 6e-8 (N = 24) to 1e-5 (N = 65) apart.  profiles/iteration_one_body.md has the figures."""
import numpy as np
import pytest
import torch

from oracle import cbind, params as P

pytestmark = pytest.mark.gpu
B = 64
OPTIMAL, MAX_ITER, INFEASIBLE = 0, 1, 2
HORIZONS = (24, 41, 65)


def _np(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items() if not k.startswith("_")}


def _both_kernels(pkg, N, out_of_box=None, **config):
    """the draw at horizon N solved by the two-wave and by the one-wave kernel: (two waves, one wave, the inputs as arrays)"""
    preset = dict(pkg.presets.barc_tracking_mpc(N), **config)
    tr = pkg.workloads.synthetic_track("barc")
    x, u = pkg.workloads.sample_initial_states("barc", B, tr["L"], [-0.01, -0.314159], [0.01, 0.314159], seed=0)
    if out_of_box is not None:
        x[out_of_box, 3] = preset["x_max"][3] + 1.0  # vx
    sv = pkg.Solver(preset, pkg.presets.barc_vehicle(), device=0)
    inp = sv.prepare(tr, x.T.copy(), 0.025)
    inp["u_ic"] = torch.as_tensor(u.T.copy(), dtype=torch.float64, device="cuda")
    sv.set_waves_per_problem(2)
    assert sv.launch_info("f64")["threads_per_problem"] == 128
    o2 = _np(sv.solve(inp))
    sv.set_waves_per_problem(1)
    assert sv.launch_info("f64")["threads_per_problem"] == 64
    o1 = _np(sv.solve(inp))
    sv.close()
    return o2, o1, _np(inp)


def _same(o2, o1, what):
    both = (o2["status"] == o1["status"]) & (o2["status"] != INFEASIBLE)
    err = {k: (np.abs((o2[k] - o1[k]) / s[:, None, None])[..., both].max() if both.any() else 0.0)
           for k, s in (("X_optm", P.SCALE_X), ("U_optm", P.SCALE_U), ("dU_optm", P.SCALE_U))}
    print("%s: statuses %s (two waves) / %s (one wave), differ on %d; iterations differ on %d (mean %.2f); X %.1e U %.1e dU %.1e on %d problems"
          % (what, np.bincount(o2["status"], minlength=3), np.bincount(o1["status"], minlength=3), (o2["status"] != o1["status"]).sum(),
             (o2["iters"] != o1["iters"]).sum(), o2["iters"].mean(), err["X_optm"], err["U_optm"], err["dU_optm"], both.sum()))
    assert np.array_equal(o2["status"], o1["status"]), np.nonzero(o2["status"] != o1["status"])[0]
    assert np.array_equal(o2["iters"], o1["iters"]), np.nonzero(o2["iters"] != o1["iters"])[0]
    assert max(err.values()) < 1e-8, err


@pytest.mark.parametrize("N", HORIZONS)
def test_out_of_box_x_ic_is_infeasible_on_exactly_those_problems(pkg, N):
    bad = np.arange(B) % 4 == 1
    o2, o1, inp = _both_kernels(pkg, N, out_of_box=bad)
    tw = cbind.solve_batch(P.barc_tracking_mpc(N), P.barc_vehicle(), inp)
    _same(o2, o1, "N = %d, vx above its bound on %d of %d" % (N, bad.sum(), B))
    for who, st in (("two waves", o2["status"]), ("one wave", o1["status"]), ("twin", tw["status"])):
        assert np.array_equal(st == INFEASIBLE, bad), (who, np.nonzero((st == INFEASIBLE) != bad)[0])


@pytest.mark.parametrize("N", HORIZONS)
def test_iteration_cap(pkg, N):
    o2, o1, _ = _both_kernels(pkg, N, max_iter=3)
    _same(o2, o1, "N = %d, max_iter = 3" % N)
    for o in (o2, o1):
        assert (o["status"] == MAX_ITER).all() and (o["iters"] == 3).all(), (np.bincount(o["status"]), np.unique(o["iters"]))
