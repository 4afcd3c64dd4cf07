"""GPU: tests/cpp/test_wave_reduce.hip -- one 64-lane wave runs every reduction of csrc/lmpc_wave.hip.h (wave_sum, wave_max,
wave_min, wave_sum_n<2> / <3>, wave_sum_split<7> / <32>, double and float) on seeded inputs, and a host re-statement of the
documented association order must give the same bits.  The `facade` target builds the program next to the library."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
LIB = Path(__file__).resolve().parents[1] / "racing-lmpc-ros2_amd" / "lib"


def test_wave_reductions_bit_for_bit():
    exe = LIB / "test_wave_reduce"
    assert exe.exists(), "run __graft_entry__.build() first"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), (r.stdout[-3000:], r.stderr[-2000:])
