"""The fused multiply-add on hybrid keys exists at every layer, checked without
a GPU: the built library exports the call, include/rnsntt.h and rns_ntt._lib
declare it with matching argument lists, and the new profile kernel has a name
at both ends."""
from __future__ import annotations

import ctypes
import os
import re

import rns_ntt
from rns_ntt import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rnt_ct_mul_relin_rescale_affine_hybrid"
PARAMS = ["rnt_buf* out0", "rnt_buf* out1", "const rnt_buf* c0", "const rnt_buf* c1", "const rnt_buf* c0p",
          "const rnt_buf* c1p", "const rnt_buf* key_a", "const rnt_buf* key_b", "size_t alpha", "int64_t w",
          "const rnt_buf* z0", "const rnt_buf* z1", "int64_t u", "int64_t bias"]
CTYPES = {"size_t": ctypes.c_size_t, "int64_t": ctypes.c_int64}


def test_library_exports_the_call():
    lib = rns_ntt.load()
    assert lib.rnt_abi_version() == 4
    assert hasattr(lib, NAME)


def test_header_and_binding_agree():
    text = open(os.path.join(REPO, "include", "rnsntt.h")).read()
    assert re.search(r"#define\s+RNT_ABI_VERSION\s+4\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", code)
    assert m, NAME
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == PARAMS
    assert NAME in text[: text.index("int " + NAME)]  # documented above its declaration
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert restype is ctypes.c_int and len(argtypes) == len(args)
    for a, t in zip(args, argtypes):  # a pointer to a buffer, or the scalar type the header names
        want = ctypes.c_void_p if "rnt_buf*" in a else CTYPES[a.split()[0]]
        assert t is want, (a, t)
    # the plain multiply's arguments come first, unchanged
    assert argtypes[:9] == _lib.SIGNATURES["rnt_ct_mul_relin_rescale_hybrid"][1]


def test_profile_name_at_both_ends():
    assert "moddown_rescale_affine" in _lib.PROFILE_NAMES
    assert '"moddown_rescale_affine"' in open(os.path.join(REPO, "include", "rnsntt.h")).read()
    src = open(os.path.join(REPO, "toy-heaan-ckks_amd", "csrc", "rnt_api.cpp")).read()
    names = re.search(r"kKernelNames\[rnt::K_COUNT\]\s*=\s*\{(.*?)\};", src, flags=re.S).group(1)
    assert tuple(re.findall(r'"(\w+)"', names)) == _lib.PROFILE_NAMES


def test_python_layers():
    for name in ("mul_ciphertexts_hybrid_rescale_affine", "poly_eval_plan_fused", "evalmod_plan", "EvalModPlan"):
        assert name in rns_ntt.__all__ and hasattr(rns_ntt, name), name
    from rns_ntt.engine import CkksEngine

    assert hasattr(CkksEngine, "eval_mod_hybrid") and hasattr(CkksEngine, "evaluate_polynomial_hybrid_fused")
