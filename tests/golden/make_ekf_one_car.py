"""Writes tests/golden/ekf_one_car.npz: one car, 50 updates of the extended Kalman filter as the numpy restatement
(tests/ekf_cases.py) computes them -- the scenario's first 25 periods for one car, with update 10 turned into a pure prediction, the
pose of update 7 dropped (NaN) and R(0,0) = 0 in update 12 (check_cov repairs it).  tests/test_gpu_ekf.py feeds the inputs to the
C++ class's driver (tests/cpp/test_ekf.cpp) and compares what it writes with x, P, K, flags here.
Run from the repository root:  python tests/golden/make_ekf_one_car.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import ekf_cases as EC  # noqa: E402

sc = EC.scenario(1, periods=25, seed=5)
cfg = dict(sc["cfg"], x0=sc["x0"][0], P0=sc["P0"][0])
f = EC.Filter(sc["veh"], cfg, 1)
f.register_observation(EC.ROWS_VEL)
f.register_observation(EC.ROWS_POSE)
f.initialize(0)
n = len(sc["updates"])
obs, ts, u = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64), np.zeros((n, 2))
z, R = np.zeros((n, 3)), np.zeros((n, 3, 3))
x, P, K, flags = np.zeros((n, 6)), np.zeros((n, 6, 6)), np.zeros((n, 6, 5)), np.zeros(n, dtype=np.int32)
for i, (o, zi, Ri, ui, ns) in enumerate(sc["updates"]):
    zi, Ri = zi.copy(), Ri.copy()
    if i == 10:
        o = -1
    if i == 7:
        zi[0, 0] = np.nan
    if i == 12:
        Ri[0, 0, 0] = 0.0
    nz = 0 if o < 0 else zi.shape[1]
    obs[i], ts[i], u[i] = o, ns, ui[0]
    z[i, :nz], R[i, :nz, :nz] = zi[0, :nz], Ri[0, :nz, :nz]
    f.update_control(ui)
    xo, Po, _, fl = f.update(o, zi if nz else None, Ri if nz else None, ns)
    x[i], P[i], K[i], flags[i] = xo[0], Po[0], f.K[0], fl[0]
assert flags[7] == EC.FALLBACK and flags[12] == EC.R_REPAIRED and np.isfinite(x).all()
np.savez(ROOT / "tests" / "golden" / "ekf_one_car.npz", x0=cfg["x0"], P0=cfg["P0"], Q=cfg["Q"], x_min=cfg["x_min"], x_max=cfg["x_max"],
         obs=obs, timestamp_ns=ts, u=u, z=z, R=R, x=x, P=P, K=K, flags=flags)
print("wrote", n, "updates; flags", flags.tolist())
