"""The call-workspace layout type (toy-heaan-ckks_amd/csrc/rnt_ws.hpp: totals,
addresses, zero-count parts, planes per ciphertext, the gadget and hybrid
scratch sized for a chunk and carved for a smaller last one, the layouts of
rnt_ct_linear_bsgs and rnt_ct_mul_relin) against hand-worked literals
(tests/cpp/test_ws_layout.cpp).  Host code: g++ alone, no HIP, no GPU; built a
second time with the address and undefined-behaviour sanitizers and run."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "cpp", "test_ws_layout.cpp")
CSRC = os.path.join(REPO, "toy-heaan-ckks_amd", "csrc")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "asan-ubsan"])
def test_ws_layout(tmp_path, flags):
    exe = str(tmp_path / "test_ws_layout")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, SRC, "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "OK (0 failures)"
