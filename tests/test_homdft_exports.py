"""ModRaise, the monomial product and the coefficient/slot transforms exist at
every layer, checked without a GPU: the built library exports rnt_mod_raise and
rnt_mul_monomial, rns_ntt._lib types them, include/rnsntt.h declares them with
exactly the documented parameters, and the package carries the engine functions
and homdft_plan."""
from __future__ import annotations

import ctypes
import inspect
import os
import re

import rns_ntt
from rns_ntt import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rnt_mod_raise": ["rnt_buf* out", "const rnt_buf* in"],
       "rnt_mul_monomial": ["rnt_buf* out", "const rnt_buf* in", "int64_t k"]}


def test_library_exports_the_calls():
    lib = rns_ntt.load()
    assert lib.rnt_abi_version() == 4  # additive: the ABI version stays
    for name in NEW:
        assert hasattr(lib, name), name


def test_binding_declares_them():
    assert _lib.SIGNATURES["rnt_mod_raise"] == (ctypes.c_int, [ctypes.c_void_p] * 2)
    assert _lib.SIGNATURES["rnt_mul_monomial"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64])
    assert "mod_raise" in _lib.PROFILE_NAMES and "mul_monomial" in _lib.PROFILE_NAMES


def test_header_declares_them():
    text = open(os.path.join(REPO, "include", "rnsntt.h")).read()
    assert re.search(r"#define\s+RNT_ABI_VERSION\s+4\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, params in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, name
        assert [" ".join(p.split()) for p in m.group(1).split(",")] == params
    # the profile names, and whether the first call of a pair can be recorded, are documented
    assert '"mod_raise"' in text and '"mul_monomial"' in text
    doc = text[text.index("ModRaise"):text.index("int rnt_mod_raise")]
    assert "CANNOT" in doc and "rnt_capture_begin" in doc


def test_profile_names_are_in_the_library_and_the_binding_table_matches_it():
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"mod_raise\x00" in blob and b"mul_monomial\x00" in blob
    for name in _lib.PROFILE_NAMES:  # the binding's table names nothing the library does not know
        assert name.encode() + b"\x00" in blob, name


def test_package_carries_the_calls():
    from rns_ntt.engine import CkksEngine

    for name in ("conjugate_hybrid", "mul_i", "split_real_imag_hybrid", "merge_real_imag", "homdft_plan"):
        assert name in rns_ntt.__all__ and callable(getattr(rns_ntt, name)), name
    assert list(inspect.signature(rns_ntt.homdft_plan).parameters) == ["degree", "direction", "depth", "order",
                                                                       "constant"]
    assert inspect.signature(rns_ntt.homdft_plan).parameters["order"].default == "bitrev"
    assert inspect.signature(rns_ntt.mul_i).parameters["sign"].default == 1
    assert list(inspect.signature(rns_ntt.RnsPoly.mod_raise).parameters) == ["self", "basis"]
    assert list(inspect.signature(rns_ntt.RnsPoly.mul_monomial).parameters) == ["self", "k"]
    for name, params in {"generate_hybrid_conjugation_key": ["self", "sk", "rng", "alpha"],
                         "conjugate_hybrid": ["ct", "conj_key"],
                         "mul_i": ["ct", "sign"],
                         "split_real_imag_hybrid": ["ct", "conj_key"],
                         "merge_real_imag": ["ct_re", "ct_im"],
                         "mod_raise": ["self", "ct", "basis"],
                         "encode_diagonal_rows_bsgs": ["diags", "baby_steps", "giant_steps", "encoder", "basis"],
                         "prepare_homdft": ["self", "plan", "top_basis"],
                         "coeff_to_slot_hybrid": ["ct", "prepared", "keysets"],
                         "slot_to_coeff_hybrid": ["ct", "prepared", "keysets"],
                         "generate_homdft_key_sets": ["self", "sk", "plan", "rng", "alpha"]}.items():
        assert list(inspect.signature(getattr(CkksEngine, name)).parameters) == params, name
    assert inspect.signature(CkksEngine.mod_raise).parameters["basis"].default is None


def test_bsgs_rescale_takes_an_output_basis():
    from rns_ntt.engine import CkksEngine

    for f in (rns_ntt.linear_transform_bsgs_hybrid_rescale, CkksEngine.linear_transform_bsgs_hybrid_rescale):
        assert inspect.signature(f).parameters["out_basis"].default is None
