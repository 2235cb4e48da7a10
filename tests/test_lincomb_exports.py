"""The scalar linear combination and the polynomial evaluator exist at every
layer, checked without a GPU: the built library exports rnt_ct_lincomb and
rnt_ct_lincomb_rescale, rns_ntt._lib types them, include/rnsntt.h declares them
with exactly the documented parameters, and the package carries ct_lincomb,
poly_eval_plan and CkksEngine.evaluate_polynomial_hybrid."""
from __future__ import annotations

import ctypes
import inspect
import os
import re

import rns_ntt
from rns_ntt import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = ["rnt_buf* out0", "rnt_buf* out1", "const rnt_buf* x0", "const rnt_buf* x1", "size_t n_in", "size_t n_out",
          "const uint64_t* weights", "const uint64_t* bias"]
NEW = {"rnt_ct_lincomb": PARAMS, "rnt_ct_lincomb_rescale": PARAMS}


def test_library_exports_the_lincomb_calls():
    lib = rns_ntt.load()
    assert lib.rnt_abi_version() == 4  # additive: the ABI version stays
    for name in NEW:
        assert hasattr(lib, name), name


def test_binding_declares_them():
    u64p = ctypes.POINTER(ctypes.c_uint64)
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == 8
        assert argtypes[:4] == [ctypes.c_void_p] * 4
        assert argtypes[4:6] == [ctypes.c_size_t, ctypes.c_size_t]
        assert argtypes[6] is u64p and argtypes[7] is u64p


def test_header_declares_them():
    text = open(os.path.join(REPO, "include", "rnsntt.h")).read()
    assert re.search(r"#define\s+RNT_ABI_VERSION\s+4\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, params in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, name
        assert [" ".join(p.split()) for p in m.group(1).split(",")] == params
    # the profile name, and whether the call can be recorded, are documented
    assert '"lincomb"' in text and "CANNOT" in text and "rnt_capture_begin" in text


def test_profile_name_is_known_without_a_device():
    # an unknown kernel name is BadArgument before any device work; a known one needs a context,
    # so the name's presence is checked in the library's string table
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"lincomb\x00" in blob


def test_package_carries_the_calls():
    from rns_ntt.engine import CkksEngine

    assert list(inspect.signature(rns_ntt.ct_lincomb).parameters)[:5] == ["ct", "n_in", "weights", "bias", "rescale"]
    assert inspect.signature(rns_ntt.ct_lincomb).parameters["rescale"].default is True
    assert inspect.signature(rns_ntt.ct_lincomb).parameters["bias"].default is None
    assert list(inspect.signature(rns_ntt.poly_eval_plan).parameters) == ["coeffs", "basis", "logp"]
    f = CkksEngine.evaluate_polynomial_hybrid
    assert list(inspect.signature(f).parameters) == ["ct", "coeffs", "rlk", "basis"]
    assert inspect.signature(f).parameters["basis"].default == "monomial"
    assert "ct_lincomb" in rns_ntt.__all__ and "poly_eval_plan" in rns_ntt.__all__
