"""The hybrid inner product exists at every layer, checked without a GPU: the
built library exports both calls, rns_ntt._lib types them, include/rnsntt.h
declares them with the documented arguments and names the new profile kernel."""
from __future__ import annotations

import ctypes
import os
import re

import rns_ntt
from rns_ntt import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rnt_ct_dot_relin_hybrid", "rnt_ct_dot_relin_rescale_hybrid")
ARGC = 10


def test_library_exports_the_dot_calls():
    lib = rns_ntt.load()
    assert lib.rnt_abi_version() == 4
    for name in NEW:
        assert hasattr(lib, name), name


def test_binding_declares_them():
    P = ctypes.c_void_p
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == ARGC
        assert argtypes[-1] is ctypes.c_size_t  # alpha
        assert argtypes[6] is ctypes.c_size_t  # n_terms
        assert all(argtypes[i] is P for i in (0, 1, 2, 3, 4, 5, 7, 8))
    assert _lib.SIGNATURES[NEW[0]][1] == _lib.SIGNATURES[NEW[1]][1]
    assert "dot_ciphertexts_hybrid" in rns_ntt.__all__ and hasattr(rns_ntt, "dot_ciphertexts_hybrid")
    from rns_ntt.engine import CkksEngine

    assert hasattr(CkksEngine, "dot_ciphertexts_hybrid")


def test_header_declares_them_and_names_the_new_profile_kernel():
    text = open(os.path.join(REPO, "include", "rnsntt.h")).read()
    assert '"dot_tensor"' in text
    assert re.search(r"#define\s+RNT_ABI_VERSION\s+4\b", text)
    assert "nine hybrid calls" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, name
        args = m.group(1).split(",")
        assert len(args) == ARGC
        assert args[-1].split() == ["size_t", "alpha"]
        assert args[6].split() == ["size_t", "n_terms"]
        assert name in text[: text.index("int " + name)]  # documented above its declaration
