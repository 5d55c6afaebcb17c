"""CPU: the sweeps' division by a launch-time divisor (differt2d_amd/csrc/d2d_div.hpp) is exact for every index below 2^31.

tests/native/d2d_div_main.cpp compares the shift and the multiply-high + correction paths with the hardware division over
the edge values; it is a stand-alone program, built here with g++ -fsanitize=undefined (an overflow or an oversized shift in
the helper ends it with a report and a non-zero status).
"""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_time_division_is_exact(tmp_path):
    exe = str(tmp_path / "d2d_div_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "d2d_div_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1"))
    assert out.returncode == 0 and out.stdout.startswith("DIV-OK"), out.stdout[-2000:] + out.stderr[-4000:]
    assert int(out.stdout.split()[1]) > 1_000_000
