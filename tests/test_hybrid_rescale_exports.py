"""The hybrid calls that end in a rescale exist at every layer, checked without
a GPU: the built library exports them, rns_ntt._lib types them and
include/rnsntt.h declares them with the documented arguments."""
from __future__ import annotations

import ctypes
import os
import re

import rns_ntt
from rns_ntt import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rnt_ct_mul_relin_rescale_hybrid": 9, "rnt_ct_linear_bsgs_hybrid_rescale": 14}  # name -> argument count


def test_library_exports_the_rescaling_hybrid_calls():
    lib = rns_ntt.load()
    assert lib.rnt_abi_version() == 4
    for name in NEW:
        assert hasattr(lib, name), name


def test_binding_declares_them():
    for name, argc in NEW.items():
        assert name in _lib.SIGNATURES, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == argc
        assert argtypes[-1] is ctypes.c_size_t  # alpha
        # the un-rescaled call's arguments
        assert argtypes == _lib.SIGNATURES[{"rnt_ct_mul_relin_rescale_hybrid": "rnt_ct_mul_relin_hybrid",
                                            "rnt_ct_linear_bsgs_hybrid_rescale": "rnt_ct_linear_bsgs_hybrid"}[name]][1]
    for name in ("mul_ciphertexts_hybrid_rescale", "linear_transform_bsgs_hybrid_rescale"):
        assert name in rns_ntt.__all__ and hasattr(rns_ntt, name)
        from rns_ntt.engine import CkksEngine

        assert hasattr(CkksEngine, name), name


def test_header_declares_them_and_names_the_new_profile_kernel():
    text = open(os.path.join(REPO, "include", "rnsntt.h")).read()
    assert '"moddown_rescale"' in text
    assert re.search(r"#define\s+RNT_ABI_VERSION\s+4\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, argc in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, name
        assert len(m.group(1).split(",")) == argc
        assert m.group(1).split(",")[-1].split() == ["size_t", "alpha"]
