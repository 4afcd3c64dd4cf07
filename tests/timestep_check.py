"""The entry points of the C ABI on the problems of tests/timestep_cases.py (a time step that differs per stage and per problem).
`solve` is what tests/test_gpu_timestep.py calls; run as a program it solves every case through lmpc_solve_batch in the default and
in the AOS result layout, holds both to the dense fixtures and to the rate identity, prints one line per case and a JSON summary and
exits 1 on any violation -- tests/test_gpu_timestep.py starts it with LMPC_HIP_LIBRARY naming the debug-hook build, the way
tests/test_gpu_dispatch.py runs its sweep in both libraries."""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import dense_cases as DC  # noqa: E402
import timestep_cases as TC  # noqa: E402

RATE_IDENTITY_TOL = 1e-12
_cases: dict = {}


def case(pkg, name: str) -> dict:
    """The fixture and its inputs, rebuilt once per process and left unchanged."""
    if name not in _cases:
        fx, cfg, veh, inp, ss_x, ss_j = TC.fixture_problems(pkg, name)
        _cases[name] = dict(fx=fx, cfg=cfg, veh=veh, inp=inp, ss_x=ss_x, ss_j=ss_j)
    return _cases[name]


def solve(pkg, name: str, entry: str = "f64", waves: int = 0, aos: bool = False, order=None) -> dict:
    """One call of an entry point on the case's problems (in the order `order`, inputs, safe sets and warm-start plans alike), numpy
    results in the default layout plus "precision", "threads" (per problem, of the fp64 cold solve) and for warm starts "accepted".
      f64       lmpc_solve_batch                         mixed     lmpc_solve_batch_mixed          f32  lmpc_solve_batch_f32
      warm      lmpc_solve_batch_warm, or for a learning case lmpc_solve_batch_warm_ss on the arrays: the plan is the fixture's optimum
      ss_idx    lmpc_solve_batch_ss_idx                  warm_idx  lmpc_solve_batch_warm_ss by reference
    (by reference: the spec laps stored on the handle, the codes from lmpc_ss_query_idx_batch)"""
    import torch

    c = case(pkg, name)
    fx, inp, ss_x, ss_j = c["fx"], c["inp"], c["ss_x"], c["ss_j"]
    plan = {k: fx[k] for k in ("X_optm", "U_optm") + (("convex_combi_optm",) if ss_x is not None else ())}
    if order is not None:
        inp, ss_x, ss_j = TC.select(inp, ss_x, ss_j, order)
        plan = {k: np.ascontiguousarray(v[..., np.asarray(order)]) for k, v in plan.items()}
    B = inp["x_ic"].shape[1]
    dev = dict(dtype=torch.float64, device="cuda")
    sv = pkg.Solver(*TC.presets(pkg, name), device=0)
    try:
        sv.reserve(B)
        if waves:
            sv.set_waves_per_problem(waves)
        if aos:
            sv.set_output_layout("aos")
        if entry == "f32":
            out = sv.solve_f32(inp)
        else:
            out = sv.alloc_outputs(B)
            kw = {}
            if ss_x is not None:
                out["convex_combi_optm"] = torch.zeros((int(c["cfg"].num_ss_pts), B), **dev)
                if entry in ("ss_idx", "warm_idx"):
                    L = float(inp["L"])
                    sv.set_safe_set(DC.spec_laps(), L)
                    kw["ss_idx"] = sv.ss_query_idx(torch.as_tensor(DC.ss_query_point(inp, L), **dev).contiguous())[0]
                else:
                    kw.update(ss_x=torch.as_tensor(ss_x, **dev), ss_j=torch.as_tensor(ss_j, **dev))
            if entry in ("warm", "warm_idx"):
                kw["warm"] = {"X_optm_ref": torch.as_tensor(plan["X_optm"], **dev), "U_optm_ref": torch.as_tensor(plan["U_optm"], **dev)}
                if ss_x is not None:
                    kw["warm"]["convex_combi_optm_ref"] = torch.as_tensor(plan["convex_combi_optm"], **dev)
            out = sv.solve(inp, out, mixed=(entry == "mixed"), **kw)
        sv.synchronize()
        res = {k: v.cpu().numpy() for k, v in out.items() if hasattr(v, "cpu")}
        res["precision"] = sv.last_solve_precision()
        res["threads"] = sv.launch_info("f64")["threads_per_problem"]
        if entry in ("warm", "warm_idx"):
            res["accepted"] = sv.warm_accepted(B).cpu().numpy()
    finally:
        sv.close()
    if aos and entry != "f32":
        for k in ("X_optm", "U_optm", "dU_optm"):
            res[k] = np.ascontiguousarray(res[k].transpose(2, 1, 0))
    return res


def check_fp64(pkg, name: str, who: str = "") -> dict:
    """lmpc_solve_batch in both result layouts: every problem status 0 and within TOL_XU / TOL_DU of the dense optimum (X, U, dU, and
    the simplex weights of a learning case); dU t_i equal to the differences of U on the entry's own outputs; the AOS call the same bits."""
    c = case(pkg, name)
    soa, aos = solve(pkg, name), solve(pkg, name, aos=True)
    exu, ed = TC.assert_matches(soa, c["fx"], "%s%s, lmpc_solve_batch" % (who, name))
    ident = TC.rate_identity_error(soa, c["inp"])
    assert ident < RATE_IDENTITY_TOL, (name, "dU t_i against the differences of U", ident)
    differ = [k for k in ("X_optm", "U_optm", "dU_optm", "convex_combi_optm", "status", "iters") if k in soa and not np.array_equal(soa[k], aos[k])]
    assert not differ, (name, "AOS layout", differ)
    return {"case": name, "xu": exu, "du": ed, "rate_identity": ident, "threads": int(soa["threads"])}


if __name__ == "__main__":
    from __graft_entry__ import load_package

    pkg = load_package()
    failures, recs = [], []
    for name in sys.argv[1:] or list(TC.CASES):
        try:
            recs.append(check_fp64(pkg, name))
        except AssertionError as e:
            failures.append({"case": name, "what": str(e)[:500]})
            print("%s   <-- %s" % (name, str(e)[:500]), flush=True)
    print(json.dumps({"library": str(pkg.library_path().name), "cases": len(recs) + len(failures), "failures": failures, "records": recs}))
    sys.exit(1 if failures else 0)
