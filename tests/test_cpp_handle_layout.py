"""The handle's I/O table (mpc_planner_amd/csrc/tmpc_handle_layout.hpp: where each input and output array of a solve lives inside the handle's two
allocations, and which handles are tick-size) checked by a stand-alone host program, tests/cpp/test_handle_layout.cpp: plain g++, the layout header
alone, built with the address and undefined-behaviour sanitizers.  Nothing touches a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_planner_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "test_handle_layout.cpp")
BIN = os.path.join(ROOT, "build", "test_handle_layout")


def _build():
    """The program, unless it is there and newer than what it is made of."""
    deps = [SRC, os.path.join(CSRC, "tmpc_handle_layout.hpp")]
    if os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in deps):
        return
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, SRC, "-o", BIN])


def test_layout_properties_and_boundary_sizes():
    _build()
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "handle layout ok" in out.stdout
