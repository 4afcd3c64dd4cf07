"""Writes tests/golden/lqr_one_car.npz: one BARC car, N = 21 at dt = 0.01, the non-symmetric weights of lqr_cases.general_config,
solved by the numpy restatement (tests/lqr_cases.py).  tests/test_lqr_reference.py reproduces it; tests/test_gpu_lqr.py feeds the
inputs to the C++ class's driver (tests/cpp/test_racing_lqr.cpp) and compares what it writes with X_optm, U_optm, K, P0 here.
Run from the repository root:  python tests/golden/make_lqr_one_car.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import lqr_cases as LC  # noqa: E402

sc = LC.scenario("barc", 21, 0.01, seed=21, B=1, general=True)
r = LC.solve(sc["veh"], sc["cfg"], sc["x_ic"], sc["X_ref"], sc["U_ref"])
assert not r["flags"].any() and np.abs(r["X_optm"] - sc["X_ref"]).max() < LC.MAX_DEVIATION["barc"]
cfg = sc["cfg"]
np.savez(ROOT / "tests" / "golden" / "lqr_one_car.npz", N=np.int32(cfg["N"]), dt=np.float64(cfg["dt"]), Q=cfg["Q"], R=cfg["R"], Qf=cfg["Qf"],
         x_ic=sc["x_ic"][0], X_ref=sc["X_ref"][0], U_ref=sc["U_ref"][0], X_optm=r["X_optm"][0], U_optm=r["U_optm"][0], K=r["K"][0], P0=r["P0"][0])
print("wrote N =", cfg["N"], "max |X_optm - X_ref| %.3f" % np.abs(r["X_optm"] - sc["X_ref"]).max())
