"""Generate tests/golden/dense_cars_<name>.npz: the dense, polished, KKT-certified optimum (oracle/qp.py `solve_dense`) of every problem
of tests/cars_model_cases.py FIXTURES on PER-CAR stage models -- oracle.dynamics.rk4_jacobian_analytic stage by stage with car b's
Vehicle, handed to build_qp(cfg, handle_vehicle, ..., lin=...), so that the boxes are the handle's -- with margin, objective,
certificate, the distance to the optimum of the same inputs on the handle's vehicle, and digests of the inputs and of the model.

It asserts, per fixture: every certificate is at most 1e-9; every optimum differs from the optimum on the handle's vehicle by more
than MIN_DISTANCE = 1e-4 (scaled X / U / dU, tests/parity.py); no problem is dropped.  A failing assertion reports the measured value;
the smallest distance seen is stored (single_vehicle_distance) and printed.  DROPPED below lists problems left out by index, with the
reason; it is empty.

Run from the repo root:  python tests/golden/make_cars_model_fixtures.py [name ...]      (CPU; about a minute)
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
import cars_model_cases as MC  # noqa: E402
from parity import per_problem_err  # noqa: E402

DROPPED = {}   # fixture name: {problem index: reason}
G = {}


def dense(job):
    b, with_model = job
    kw = {} if G["ss_x"] is None else {"ss_x": G["ss_x"][:, :, b], "ss_j": G["ss_j"][:, b]}
    if with_model:
        kw["lin"] = tuple(m[b] for m in G["model"])
    qp = Q.build_qp(G["cfg"], G["veh"], S.problem(G["inp"], b), **kw)
    y, info = Q.solve_dense(qp)
    o = qp.split(y)
    c = Q.kkt_certificate(qp, y)
    gs = max(1.0, float(np.abs(qp.H @ y + qp.h).max()))
    return (info["status"], bool(info.get("polished")), o["X_optm"], o["U_optm"], o["dU_optm"], Q.strict_complementarity(qp, y, info["lam"]),
            qp.objective(y), (c["stat"] / gs, c["eq"], c["ineq"], c["comp"]))


if __name__ == "__main__":
    pkg = load_package()
    for name in sys.argv[1:] or list(MC.FIXTURES):
        cfg, veh, inp, ss_x, ss_j, table = MC.build(pkg, name)
        model = MC.qp_model(MC.reference(inp, table))
        G.update(cfg=cfg, veh=veh, inp=inp, ss_x=ss_x, ss_j=ss_j, model=model)
        B, N = inp["x_ic"].shape[-1], cfg.N
        t0 = time.time()
        with ProcessPoolExecutor(min(16, os.cpu_count())) as ex:
            res = list(ex.map(dense, [(b, True) for b in range(B)] + [(b, False) for b in range(B)], chunksize=2))
        per_car, handle = res[:B], res[B:]
        status = np.array([r[0] for r in per_car], dtype=np.int32)
        cert = np.array([r[7] for r in per_car])
        stack = lambda rs: {k: np.stack([r[i] for r in rs], -1) for i, k in ((2, "X_optm"), (3, "U_optm"), (4, "dU_optm"))}   # noqa: E731
        opt, single = stack(per_car), stack(handle)
        exu, ed = per_problem_err(opt, single)
        dist = np.maximum(exu, ed)
        print(f"dense_{name}: {B} problems (N = {N}), solved {(status == 0).sum()}, polished {sum(r[1] for r in per_car)}; certificate worst "
              f"{cert.max():.1e}; distance to the optimum on the handle's vehicle min {dist.min():.1e} (problem {int(np.argmin(dist))}) max "
              f"{dist.max():.1e}; per kind min {[float('%.1e' % dist[k::3].min()) for k in range(3)]}  ({time.time() - t0:.0f} s)", flush=True)
        assert not DROPPED.get(name), "a dropped problem changes the fixture's problem list: slice it out here, by index, with its reason"
        assert (status == 0).all() and all(r[0] == 0 for r in handle), (name, "not solved", np.nonzero(status)[0])
        assert cert.max() <= MC.MAX_CERTIFICATE, (name, "certificate", cert.max(), np.argmax(cert.max(axis=1)))
        assert dist.min() > MC.MIN_DISTANCE, (name, "distance to the optimum on the handle's vehicle", dist.min(), int(np.argmin(dist)))
        d_in, d_model = MC.digest(inp, ss_x, ss_j, model)
        np.savez_compressed(ROOT / "tests" / "golden" / f"dense_{name}.npz", status=status, polished=np.array([r[1] for r in per_car]), **opt,
                            margin=np.array([r[5] for r in per_car]), objective=np.array([r[6] for r in per_car]), kkt_cert=cert.T,
                            single_vehicle_distance=dist, digest=d_in, model_digest=d_model)
