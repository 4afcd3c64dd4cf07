"""The stage chains on explicit LDS byte addresses (csrc/lmpc_solve_layout.hip.h `lmpc_chain_addr`: the fp64 tracking kernels of
N <= 23 -- cold, warm and the second pass of a mixed solve).  Only how an address is formed changes there, so what can go wrong is an
address: a pattern that starts one cell or one stage off, a stride with the wrong sign, the one-stage-ahead fetch running past the
first or the last stage, a dead-cell store that walks.  Any of these gives a wrong Newton step, and the solve then ends somewhere
else or not at all -- so fp64 BARC tracking, 256 problems, against the serial twin with what tests/dispatch_sweep.py asks of a case
(statuses equal but for at most two borderline polish acceptances and never INFEASIBLE against anything else, X / U within TOL_TWIN
and dU within TOL_DU scaled, iteration counts equal on >= 90 % and never more than 8 apart, solved fraction):
  * N = 3 (two stages: the fetch ahead is clamped from the first stage on), 11 | 12 (KQ = 2 | 4), 20 (the benchmark's), 23 (the last
    of the class), each with the shared boundary slack (two right-hand sides, the backward sweep inside the factorisation) and
    without (one right-hand side, both sweeps in the vector solve);
  * a warm solve and a mixed solve whose fp64 second pass runs: kernels of their own over the same loops;
  * N = 24: the first horizon outside the class, whose kernel keeps the form it had."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import cbind, params as P
from tolerances import TOL_DU, TOL_TWIN

pytestmark = pytest.mark.gpu
SX, SU = P.SCALE_X[:, None, None], P.SCALE_U[:, None, None]
B = 256


def _np(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items() if not k.startswith("_")}


def _case(pkg, N, slack=True, polish=None):
    """the dispatch sweep's BARC tracking draw at horizon N: solver, prepared inputs, the twin's configuration"""
    cfg, preset = P.barc_tracking_mpc(N), dict(pkg.presets.barc_tracking_mpc(N))
    if not slack:
        cfg = dataclasses.replace(cfg, q_boundary=0.0)
        preset["q_boundary"] = 0.0
    if polish is not None:
        preset["polish"] = polish
    tr = pkg.workloads.synthetic_track("barc")
    x, u = pkg.workloads.sample_initial_states("barc", B, tr["L"], [-0.01, -0.314159], [0.01, 0.314159], seed=0)
    sv = pkg.Solver(preset, pkg.presets.barc_vehicle(), device=0)
    sv.reserve(B)
    inp = sv.prepare(tr, x.T.copy(), 0.025)
    inp["u_ic"] = torch.as_tensor(u.T.copy(), dtype=torch.float64, device="cuda")
    return sv, inp, cfg


def _against_the_twin(o, tw, N, what, among=None, min_solved=None):
    """tests/dispatch_sweep.py `one`, the fp64 part, on the problems `among` (default: all)"""
    among = np.ones(o["status"].shape, bool) if among is None else among
    ok = (o["status"] == 0) & (tw["status"] == 0) & among
    differ = np.nonzero((o["status"] != tw["status"]) & among)[0]
    exu = max(np.abs((o["X_optm"] - tw["X_optm"]) / SX)[..., ok].max(), np.abs((o["U_optm"] - tw["U_optm"]) / SU)[..., ok].max()) if ok.any() else 0.0
    edu = np.abs((o["dU_optm"] - tw["dU_optm"]) / SU)[..., ok].max() if ok.any() else 0.0
    di = np.abs(o["iters"][ok] - tw["iters"][ok])
    print("%s: solved %d of %d, statuses differ on %d, X/U %.1e, dU %.1e, iterations equal %.3f (mean %.2f, max difference %d)"
          % (what, ok.sum(), among.sum(), differ.size, exu, edu, (di == 0).mean() if ok.any() else 1.0, o["iters"][ok].mean() if ok.any() else 0.0,
             di.max() if ok.any() else 0))
    assert differ.size <= 2 and not ((o["status"][differ] == 2) | (tw["status"][differ] == 2)).any(), (differ[:6], o["status"][differ[:6]], tw["status"][differ[:6]])
    assert exu < TOL_TWIN and edu < TOL_DU, (exu, edu)
    assert ok.any() and (di == 0).mean() >= 0.9 and di.max() <= 8, ((di == 0).mean(), di.max())
    floor = (0.95 if N >= 6 else 0.5) if min_solved is None else min_solved
    assert ok.sum() >= floor * among.sum(), (ok.sum(), among.sum())


@pytest.mark.parametrize("N,slack", [(N, s) for N in (3, 11, 12, 20, 23) for s in (True, False)] + [(24, True)])
def test_cold_solve_against_the_twin(pkg, N, slack):
    sv, inp, cfg = _case(pkg, N, slack)
    o = _np(sv.solve(inp))
    tw = cbind.solve_batch(cfg, P.barc_vehicle(), _np(inp))
    sv.close()
    # (without the slack a start outside the track at knot 0 has no feasible point: the dispatch sweep's solved fraction is a
    #  statement about the draw with the slack; statuses must agree all the same)
    _against_the_twin(o, tw, N, "N = %d, %s" % (N, "shared slack" if slack else "hard boundary"), min_solved=None if slack else 0.0)


def test_warm_solve_against_the_twin(pkg):
    """lmpc_solve_warm_kernel<4, 0> with the linearisation trajectory as the plan: accepted where the active-set attempt holds, the
    interior point from the cold start (the stage chains, in the warm kernel) where it does not."""
    sv, inp, cfg = _case(pkg, 20)
    o = _np(sv.solve(inp, warm=True))
    acc = sv.warm_accepted(B).cpu().numpy()
    tw = cbind.solve_batch(cfg, P.barc_vehicle(), _np(inp), warm=True)
    sv.close()
    print("warm attempts accepted: %d of %d" % (acc.sum(), B))
    assert (acc == 0).sum() >= B // 8   # the chains ran
    _against_the_twin(o, tw, 20, "N = 20, warm")


def test_second_pass_of_a_mixed_solve_against_the_twin(pkg):
    """lmpc_cleanup_kernel<double, 4, 0, double>: the problems the fp32 pass leaves unverified (found with polish = 1: one pass, they
    keep LMPC_SOLVE_UNVERIFIED) are solved by the fp64 second pass of the default two-pass solve."""
    sv1, inp, cfg = _case(pkg, 20, polish=1)
    one = _np(sv1.solve(inp, mixed=True))
    assert sv1.last_solve_precision() == "mixed"
    sv1.close()
    marked = one["status"] == 3
    sv, inp, cfg = _case(pkg, 20)
    two = _np(sv.solve(inp, mixed=True))
    assert sv.last_solve_precision() == "mixed"
    sv.close()
    tw = cbind.solve_batch(cfg, P.barc_vehicle(), _np(inp))
    print("left to the second pass: %d of %d" % (marked.sum(), B))
    assert marked.sum() >= 8 and not (two["status"] == 3).any()
    _against_the_twin(two, tw, 20, "N = 20, second pass", among=marked)
