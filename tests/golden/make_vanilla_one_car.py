"""Writes tests/golden/vanilla_one_car.npz: one BARC car of the "barc" scenario of tests/vanilla_cases.py, 64 control periods of
controller + plant by the numpy restatement (vanilla_cases.rollout), and the same 64 decisions taken one at a time on the logged
states with the reference speed passed explicitly (vanilla_cases.decide, the PID state carried).  tests/test_vanilla_reference.py
reproduces it; tests/test_gpu_vanilla.py feeds x_ic = X_log[:, p] and vel_ref[p] to the C++ class's driver
(tests/cpp/test_vanilla_controller.cpp) and compares what it writes with the C ABI at B = 1 and with u_out here.
Run from the repository root:  python tests/golden/make_vanilla_one_car.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import vanilla_cases as VC  # noqa: E402

sc = VC.scenario("barc", B=1)
P = VC.PERIODS
r = VC.rollout(sc["veh"], sc["cfg"], sc["trk"], sc["x0"], VC.zero_pid(1), P, sc["dt_sim"], sc["n_sub"], sc["speed_scale"])
assert not r["flags"].any() and r["worst_excess"].max() <= 0.0
pid = VC.zero_pid(1)
u_out, vel_ref = np.empty((P, 3)), np.empty(P)
for p in range(P):
    x = r["X_log"][:, :, p]
    vel_ref[p] = VC.spline_eval(sc["trk"]["spline"], x[:, 0], np.float64)["vel"][0] * sc["speed_scale"]
    d = VC.decide(sc["veh"], sc["cfg"], sc["trk"], x, pid, vel_ref[p:p + 1])
    assert np.array_equal(d["u_model"], r["U_log"][:, :, p])
    u_out[p], pid = d["u_out"][0], d["pid"]
cfg = sc["cfg"]
names = sorted(cfg)
np.savez(ROOT / "tests" / "golden" / "vanilla_one_car.npz", cfg_names=np.array(names), cfg_values=np.array([cfg[k] for k in names]),
         dt_sim=np.float64(sc["dt_sim"]), n_sub=np.int32(sc["n_sub"]), speed_scale=np.float64(sc["speed_scale"]), x0=sc["x0"][0],
         x=r["x"][0], X_log=r["X_log"][0], U_log=r["U_log"][0], k_log=r["k_log"][0], distance=r["distance"][0],
         worst_excess=r["worst_excess"][0], pid=np.array([r["pid"][k][0] for k in VC.PID_KEYS]), vel_ref=vel_ref, u_out=u_out)
print("wrote", P, "periods; distance %.3f m, worst_excess %.4f" % (r["distance"][0], r["worst_excess"][0]))
