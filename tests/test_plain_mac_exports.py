"""The plaintext multiply-accumulate exists at every layer, checked without a
GPU: the built library exports rnt_ct_plain_mac and rnt_ct_plain_mac_rescale,
rns_ntt._lib types them, include/rnsntt.h declares and documents them and names
the new profile kernel, and the package carries the Python functions."""
from __future__ import annotations

import ctypes
import os
import re

import rns_ntt
from rns_ntt import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rnt_ct_plain_mac", "rnt_ct_plain_mac_rescale")
PARAMS = ["rnt_buf* out0", "rnt_buf* out1", "const rnt_buf* x0", "const rnt_buf* x1", "const rnt_buf* m",
          "const rnt_buf* bias", "size_t n_terms"]


def test_library_exports_both_calls():
    lib = rns_ntt.load()
    assert lib.rnt_abi_version() == 4
    for name in NAMES:
        assert hasattr(lib, name), name


def test_header_and_binding_agree():
    text = open(os.path.join(REPO, "include", "rnsntt.h")).read()
    assert re.search(r"#define\s+RNT_ABI_VERSION\s+4\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, name
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == PARAMS
        assert name in text[: text.index("int " + name + "(")]  # documented above its declaration
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == 7
        assert all(t is ctypes.c_void_p for t in argtypes[:6]) and argtypes[6] is ctypes.c_size_t
    # the header's error table names every status the calls return
    section = text[text.index("ciphertext x plaintext multiply-accumulate"): text.index("int rnt_ct_plain_mac_rescale(")]
    for status in ("RNT_ERR_BAD_ARGUMENT", "RNT_ERR_BASIS_MISMATCH", "RNT_ERR_DOMAIN_MISMATCH", "RNT_ERR_UNSUPPORTED",
                   "RNT_ERR_INVALID_MOD_DROP"):
        assert status in section, status
    assert "word for word" in section


def test_profile_name_at_both_ends():
    assert _lib.PROFILE_NAMES[-1] == "plain_mac"
    assert '"plain_mac"' in open(os.path.join(REPO, "include", "rnsntt.h")).read()
    src = open(os.path.join(REPO, "toy-heaan-ckks_amd", "csrc", "rnt_api.cpp")).read()
    names = re.search(r"kKernelNames\[rnt::K_COUNT\]\s*=\s*\{(.*?)\};", src, flags=re.S).group(1)
    assert tuple(re.findall(r'"(\w+)"', names)) == _lib.PROFILE_NAMES


def test_python_layers():
    for name in ("ct_plain_mac", "mul_plain"):
        assert name in rns_ntt.__all__ and callable(getattr(rns_ntt, name)), name
    from rns_ntt.engine import CkksEngine

    for name in ("prepare_plaintext", "mul_plaintext", "plain_mac", "add_plaintext"):
        assert callable(getattr(CkksEngine, name)), name
