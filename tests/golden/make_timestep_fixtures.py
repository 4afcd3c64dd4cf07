"""Generate tests/golden/dense_dt_<case>.npz: the dense, polished, KKT-certified optimum (oracle/qp.py `solve_dense`) of every problem
of tests/timestep_cases.py -- the suite's problem sets on a time step that differs per stage and per problem -- together with the
optimum of the same problem with T_ref rolled by one stage and the scaled distance between the two.

Asserted here (and again by tests/test_timestep_fixtures.py on the committed files), per case:
  * every stored problem has dense status 0 and a KKT certificate; a problem the dense solver cannot certify is replaced by the next
    one of the draw, at most 10 % of the case;
  * at least a quarter of the problems have a rate row (dU at its box) active at some stage, read from the dense multipliers;
  * the rolled-T_ref optimum is at least 1e3 TOL_XU (scaled) from the true one on every problem.

Run from the repo root:  python tests/golden/make_timestep_fixtures.py [case ...]      (CPU; a few minutes on 8 cores for all)
"""
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor
from pathlib import Path

os.environ.setdefault("OMP_NUM_THREADS", "1")
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
import numpy as np  # noqa: E402

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from __graft_entry__ import load_package  # noqa: E402
from oracle import params as P, qp as Q, scenario as S  # noqa: E402
import dense_cases as DC  # noqa: E402
import timestep_cases as TC  # noqa: E402

G = {}
KEYS = ("X_optm", "U_optm", "dU_optm")


def _solve(inp, b):
    kw = {} if G["ss_x"] is None else {"ss_x": G["ss_x"][:, :, b], "ss_j": G["ss_j"][:, b]}
    qp = Q.build_qp(G["cfg"], G["veh"], S.problem(inp, b), **kw)
    try:
        y, info = Q.solve_dense(qp)
    except np.linalg.LinAlgError:
        return None
    c = Q.kkt_certificate(qp, y)
    gs = max(1.0, float(np.abs(qp.H @ y + qp.h).max()))
    return qp, y, info, (c["stat"] / gs, c["eq"], c["ineq"], c["comp"])


def save_npz(path, **arrays):
    """np.savez without the clock: zip members stamped 1980-01-01, so that a second run writes the same bytes."""
    import zipfile

    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for k, v in arrays.items():
            with z.open(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)


def certified(status, cert) -> bool:
    return status == 0 and cert[0] < 1e-9 and cert[1] < 1e-9 and cert[2] < 1e-9 and cert[3] < 1e-8


def dense(b):
    """Problem b of the pool and its rolled twin -> None where either is not certified."""
    r, rr = _solve(G["inp"], b), _solve(G["rolled"], b)
    if r is None or rr is None or not certified(r[2]["status"], r[3]) or rr[2]["status"] != 0:
        return None
    qp, y, info, cert = r
    o, orl = qp.split(y), rr[0].split(rr[1])
    dist = max(np.abs((o["X_optm"] - orl["X_optm"]) / P.SCALE_X[:, None]).max(), np.abs((o["U_optm"] - orl["U_optm"]) / P.SCALE_U[:, None]).max(),
               np.abs((o["dU_optm"] - orl["dU_optm"]) / P.SCALE_U[:, None]).max())
    return {"o": o, "rolled": orl, "dist": dist, "cert": cert, "polished": bool(info.get("polished")), "iters": info["iters"],
            "margin": Q.strict_complementarity(qp, y, info["lam"]), "objective": qp.objective(y), "rate": TC.rate_row_active(qp, info["lam"])}


if __name__ == "__main__":
    pkg = load_package()
    names = sys.argv[1:] or list(TC.CASES)
    for name in names:
        cfg, veh, inp, ss_x, ss_j = TC.build(pkg, name)
        G.update(cfg=cfg, veh=veh, inp=inp, rolled=TC.rolled(inp), ss_x=ss_x, ss_j=ss_j)
        count, pool, N = TC.CASES[name][2], TC.pool_size(name), cfg.N
        t0 = time.time()
        with ProcessPoolExecutor(min(8, os.cpu_count())) as ex:
            res = list(ex.map(dense, range(pool)))
        good = [b for b, r in enumerate(res) if r is not None]
        assert 0 in good, (name, "problem 0 (the structured T_ref) is not certified")
        idx = np.array(good[:count])
        replaced = int((idx >= count).sum())
        assert idx.size == count and replaced <= TC.REPLACED_SHARE_MAX * count, (name, "problems the dense solver could not certify", sorted(set(range(count)) - set(good)))
        sel = [res[b] for b in idx]
        rate_share = float(np.mean([r["rate"] for r in sel]))
        dist = np.array([r["dist"] for r in sel])
        print(f"dense_{name}: {count} problems (N = {N}), replaced {replaced}, active rate row on {100 * rate_share:.0f} %, rolled-T_ref distance "
              f"min {dist.min():.2e} max {dist.max():.2e}, certificate worst {np.array([r['cert'] for r in sel]).max(axis=0)}, "
              f"polished {sum(r['polished'] for r in sel)}  ({time.time() - t0:.0f} s)", flush=True)
        assert rate_share >= TC.ACTIVE_RATE_SHARE_MIN, (name, rate_share)
        assert dist.min() >= TC.SENSITIVITY_MIN, (name, dist.min())
        sinp, sx, sj = TC.select(inp, ss_x, ss_j, idx)
        extra = {}
        if ss_x is not None:
            extra["convex_combi_optm"] = np.stack([r["o"]["convex_combi_optm"] for r in sel], -1)
        save_npz(ROOT / "tests" / "golden" / f"dense_{name}.npz",
                 status=np.zeros(count, dtype=np.int32), polished=np.array([r["polished"] for r in sel]), draw_index=idx.astype(np.int32),
                 **{k: np.stack([r["o"][k] for r in sel], -1) for k in KEYS}, **{k + "_rolled": np.stack([r["rolled"][k] for r in sel], -1) for k in KEYS},
                 sigma=np.array([r["o"].get("sigma", 0.0) for r in sel]), rolled_distance=dist, rate_row_active=np.array([r["rate"] for r in sel]),
                 margin=np.array([r["margin"] for r in sel]), objective=np.array([r["objective"] for r in sel]),
                 kkt_cert=np.array([r["cert"] for r in sel]).T, iters=np.array([r["iters"] for r in sel], dtype=np.int32),
                 T_ref=sinp["T_ref"], digest=DC.digest(sinp, sx, sj), **extra)
