"""The row phases of the solve kernels on wave reductions that carry no identity operand (csrc/lmpc_wave.hip.h: `wave_reduce_n`,
`pair_exchange`; csrc/lmpc_knn_select.hip.h).  A lane the DPP does not write now holds an unspecified value, so what can go wrong
is a reader of such a lane: a wrong mu, step length, Schur sum or polish vote.  Any of these ends a solve somewhere else or not at
all -- so every user of the reductions, 256 problems each, against the serial twin with the draw, the criteria and the tolerances
of tests/test_gpu_chain_addresses.py and tests/dispatch_sweep.py (statuses equal but for at most two borderline polish
acceptances, X / U within TOL_TWIN and dU within TOL_DU scaled, iteration counts equal on >= 90 % and never more than 8 apart,
solved fraction; the fp32 and mixed entries against the fp64 kernel's answers at TOL_F32_SWEEP, nothing lost, nothing unverified):
  * cold fp64 at N = 3, 12, 20 and 24: KQ = 2, 4, 4 and 7 slots per lane (`wave_sum_n<2>`, `<3>`, `wave_max`, `wave_min`);
  * the learning problem at N = 20 with 96 and with 160 safe-set points: `wave_sum_split<32>`, `<7>`, `<3>`, in fp64 and in the
    mixed entry's fp32 kernels;
  * a mixed solve at N = 20 whose fp64 second pass runs;
  * fp32 IAC at N = 40: the reductions in `float`;
  * N = 41: two waves per problem, every exchange a `wave_reduce_n` and two LDS cells (csrc/lmpc_solve_w2.hip.h)."""
import numpy as np
import pytest

import dispatch_sweep as DS
import test_gpu_chain_addresses as CA
from oracle import cbind, params as P

pytestmark = pytest.mark.gpu
B = CA.B


@pytest.mark.parametrize("N", [3, 12, 20, 24])
def test_cold_solve_against_the_twin(pkg, N):
    sv, inp, cfg = CA._case(pkg, N)
    o = CA._np(sv.solve(inp))
    tw = cbind.solve_batch(cfg, P.barc_vehicle(), CA._np(inp))
    sv.close()
    CA._against_the_twin(o, tw, N, "N = %d" % N)


def _sweep_case(family, N):
    failures = []
    rec = DS.one(family, N, B, failures)
    assert not failures, failures
    return rec


@pytest.mark.parametrize("family", ["lrn96", "lrn160"])
def test_learning_problem_against_the_twin(pkg, family):
    rec = _sweep_case(family, 20)
    assert "mixed" in rec   # the fp32 kernels of the mixed entry ran as well


def test_second_pass_of_a_mixed_solve_against_the_twin(pkg):
    sv1, inp, cfg = CA._case(pkg, 20, polish=1)
    marked = CA._np(sv1.solve(inp, mixed=True))["status"] == 3
    sv1.close()
    sv, inp, cfg = CA._case(pkg, 20)
    two = CA._np(sv.solve(inp, mixed=True))
    assert sv.last_solve_precision() == "mixed"
    sv.close()
    tw = cbind.solve_batch(cfg, P.barc_vehicle(), CA._np(inp))
    print("left to the second pass: %d of %d" % (marked.sum(), B))
    assert marked.sum() >= 8 and not (two["status"] == 3).any()
    CA._against_the_twin(two, tw, 20, "N = 20, second pass", among=marked)


def test_fp32_iac_against_the_twin(pkg):
    rec = _sweep_case("iac", 40)
    assert "f32" in rec and "mixed" in rec


def test_two_waves_against_the_twin(pkg):
    sv = pkg.Solver(pkg.presets.barc_tracking_mpc(41), pkg.presets.barc_vehicle(), device=0)
    assert sv.launch_info("f64")["threads_per_problem"] == 128
    sv.close()
    _sweep_case("trk", 41)
