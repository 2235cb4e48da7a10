"""The launch geometry the streaming launchers share
(toy-heaan-ckks_amd/csrc/rnt_launch.hpp: the 16-byte predicate, grid x, the
limb split, tier / flag / word dispatch) against hand-worked literals
(tests/cpp/test_launch_geom.cpp).  Host code: g++ alone, no HIP, no GPU."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "cpp", "test_launch_geom.cpp")
CSRC = os.path.join(REPO, "toy-heaan-ckks_amd", "csrc")


def test_launch_geometry_helpers(tmp_path):
    exe = str(tmp_path / "test_launch_geom")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, SRC, "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "OK (0 failures)"
