"""The active-set polish and the start point of the fp64 tracking kernels of N <= 23 on explicit LDS byte addresses
(csrc/lmpc_solve_layout.hip.h `lmpc_chain_addr`): the polish's factorisation and vector solves, the start point's factorisation and
`feedback_rollout`, which under the policy has the forward sweep's form (z_i in one register per lane, everything else fetched one
stage ahead).  As in tests/test_gpu_chain_addresses.py, what can go wrong is an address -- a pattern one cell or one stage off, a
fetch ahead that runs past the last stage, a dead-cell store that walks -- and the solve then ends somewhere else or not at all.  So
the same draw (256 problems, seed 0), the same criteria against the serial twin and the same tolerances:
  * cold solves at N = 3 (two stages: every fetch ahead is clamped from the first stage), 11 | 12 (KQ = 2 | 4), 20, 23, each with the
    shared boundary slack and without (q_boundary = 0: the polish's first step has one right-hand side), and N = 24, the first horizon
    outside the class;
  * each of them once more with the polish switched off (the preset's polish = -1): the iteration counts must differ from the solve
    with the polish on at least 80 % of the problems both solve -- the polish ran, and the agreement above is about its code (the
    twin's counts differ on 94 .. 99 % of the solved problems of this draw at the ten cases of the class, 186 of 197 at the least);
  * a warm solve with the linearisation trajectory as the plan (`feedback_rollout<true>` and the warm kernel's polish);
  * a default mixed solve whose fp64 second pass runs (the cleanup kernel's polish)."""
import numpy as np
import pytest

from oracle import cbind, params as P
from test_gpu_chain_addresses import B, _against_the_twin, _case, _np

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,slack", [(N, s) for N in (3, 11, 12, 20, 23) for s in (True, False)] + [(24, True)])
def test_cold_solve_against_the_twin_and_the_polish_ran(pkg, N, slack):
    what = "N = %d, %s" % (N, "shared slack" if slack else "hard boundary")
    sv, inp, cfg = _case(pkg, N, slack)
    o = _np(sv.solve(inp))
    sv.close()
    sv, inp_off, _ = _case(pkg, N, slack, polish=-1)
    off = _np(sv.solve(inp_off))
    sv.close()
    tw = cbind.solve_batch(cfg, P.barc_vehicle(), _np(inp))
    both = (o["status"] == 0) & (off["status"] == 0)
    moved = o["iters"][both] != off["iters"][both]
    print("%s: polish on / off both solve %d, iteration counts differ on %d (%.3f)" % (what, both.sum(), moved.sum(), moved.mean() if both.any() else 0.0))
    _against_the_twin(o, tw, N, what, min_solved=None if slack else 0.0)
    assert both.any() and moved.mean() >= 0.8, (moved.sum(), both.sum())


def test_warm_solve_against_the_twin(pkg):
    """lmpc_solve_warm_kernel<4, 0>: the plan rolled out by `feedback_rollout<true>`, the active-set attempt by the polish the warm
    kernel keeps inline; refused attempts go on through the cold start (start factorisation, `feedback_rollout<false>`)."""
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
    keep LMPC_SOLVE_UNVERIFIED) are solved, start point and polish included, by the fp64 second pass of the default two-pass solve."""
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
