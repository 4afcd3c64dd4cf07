"""Generate tests/golden/dense_reg_<case>.npz: the dense, polished optimum (oracle/qp.py `solve_dense`) of every problem of
tests/dense_cases.py REG_CASES on the ORACLE's regressed stage models (oracle.qp.linearise + oracle.regression.regress_batch,
handed to build_qp(lin=...)), with margin, objective, boundary slack, the KKT certificate of the point stored, and digests of the inputs, of the
regression samples and of the corrected model.

Run from the repo root:  python tests/golden/make_reg_dense_fixtures.py [case ...]      (CPU; about a minute on 8 cores)
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
from oracle import qp as Q, scenario as S  # noqa: E402
import dense_cases as DC  # noqa: E402

G = {}


def dense(b):
    A, B, g = (m[b] for m in G["model"][:3])
    kw = {} if G["ss_x"] is None else {"ss_x": G["ss_x"][:, :, b], "ss_j": G["ss_j"][:, b]}
    qp = Q.build_qp(G["cfg"], G["veh"], S.problem(G["inp"], b), lin=(A, B, g), **kw)
    try:
        y, info = Q.solve_dense(qp)
    except np.linalg.LinAlgError:
        return None
    o = qp.split(y)
    if info["status"] != 0 or not np.isfinite(y).all():   # no optimum: the status is the fixture's content, the answer slots are NaN
        nan = np.nan
        return (info["status"] if info["status"] != 0 else 1, False, np.full_like(o["X_optm"], nan), np.full_like(o["U_optm"], nan),
                np.full_like(o["dU_optm"], nan), nan, nan, (nan, nan, nan, nan), nan)
    c = Q.kkt_certificate(qp, y)
    gs = max(1.0, float(np.abs(qp.H @ y + qp.h).max()))
    return (info["status"], bool(info.get("polished")), o["X_optm"], o["U_optm"], o["dU_optm"], Q.strict_complementarity(qp, y, info["lam"]),
            qp.objective(y), (c["stat"] / gs, c["eq"], c["ineq"], c["comp"]), float(o.get("sigma", 0.0)))


if __name__ == "__main__":
    pkg = load_package()
    names = sys.argv[1:] or list(DC.REG_CASES)
    for name in names:
        cfg, veh, inp, ss_x, ss_j, samples, spec, model = DC.build_reg(pkg, name)
        G.update(cfg=cfg, veh=veh, inp=inp, ss_x=ss_x, ss_j=ss_j, model=model)
        B, N = inp["x_ic"].shape[-1], cfg.N
        t0 = time.time()
        with ProcessPoolExecutor(os.cpu_count()) as ex:
            res = list(ex.map(dense, range(B), chunksize=2))
        bad = [b for b, r in enumerate(res) if r is None]
        assert not bad, (name, "singular KKT system", bad)
        st = np.array([r[0] for r in res], dtype=np.int32)
        md, sd = DC.reg_digests(samples, model)
        np.savez_compressed(ROOT / "tests" / "golden" / f"dense_{name}.npz",
                            status=st, polished=np.array([r[1] for r in res]), X_optm=np.stack([r[2] for r in res], -1),
                            U_optm=np.stack([r[3] for r in res], -1), dU_optm=np.stack([r[4] for r in res], -1),
                            margin=np.array([r[5] for r in res]), objective=np.array([r[6] for r in res]),
                            kkt_cert=np.array([r[7] for r in res]).T, sigma=np.array([r[8] for r in res]), digest=DC.digest(inp, ss_x, ss_j), model_digest=md,
                            samples_digest=np.float64(sd), touched=model[3].sum(axis=1))
        cert = np.array([r[7] for r in res])[st == 0]
        print(f"dense_{name}: {B} problems (N = {N}), solved {(st == 0).sum()}, polished {sum(r[1] for r in res)}, stages regressed "
              f"{model[3].sum()} of {model[3].size}; certificate worst: stationarity {cert[:, 0].max():.1e} (relative) rows "
              f"{max(cert[:, 1].max(), cert[:, 2].max()):.1e} complementarity {cert[:, 3].max():.1e}  ({time.time() - t0:.0f} s)", flush=True)
