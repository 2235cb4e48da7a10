"""Key level views (one full-level hybrid key at every level) exist at every
layer, checked without a GPU: the built library exports rnt_ctx_hybrid_level and
rnt_key_level_view, rns_ntt._lib types them, include/rnsntt.h declares them and
the package carries RnsBasis.hybrid_level and the two at_level methods."""
from __future__ import annotations

import ctypes
import inspect
import os
import re

import rns_ntt
from rns_ntt import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {  # name -> the C parameters
    "rnt_ctx_hybrid_level": ["const rnt_ctx* key_ctx", "size_t n_special", "size_t level", "rnt_ctx** out"],
    "rnt_key_level_view": ["const rnt_buf* key", "const rnt_ctx* level_ctx", "size_t alpha", "rnt_buf** out"],
}


def test_library_exports_the_level_calls():
    lib = rns_ntt.load()
    assert lib.rnt_abi_version() == 4
    for name in NEW:
        assert hasattr(lib, name), name


def test_binding_declares_them():
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == 4
    assert _lib.SIGNATURES["rnt_ctx_hybrid_level"][1][1:3] == [ctypes.c_size_t, ctypes.c_size_t]
    assert _lib.SIGNATURES["rnt_key_level_view"][1][2] is ctypes.c_size_t


def test_header_declares_them():
    text = open(os.path.join(REPO, "include", "rnsntt.h")).read()
    assert re.search(r"#define\s+RNT_ABI_VERSION\s+4\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, params in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, name
        assert [" ".join(p.split()) for p in m.group(1).split(",")] == params
    # the two lifetime rules of a view are documented
    assert "must outlive its views" in text and "re-preparing" in text


def test_package_carries_the_level_methods():
    assert callable(getattr(rns_ntt.RnsBasis, "hybrid_level", None))
    assert list(inspect.signature(rns_ntt.RnsBasis.hybrid_level).parameters) == ["self", "n_special", "level"]
    assert callable(getattr(rns_ntt.RnsHybridKey, "at_level", None))
    assert list(inspect.signature(rns_ntt.RnsHybridKey.at_level).parameters) == ["self", "level", "n_special"]
    assert callable(getattr(rns_ntt.RnsHybridKeySet, "at_level", None))
    assert list(inspect.signature(rns_ntt.RnsHybridKeySet.at_level).parameters) == ["self", "level"]
    assert "n_special" in inspect.signature(rns_ntt.RnsHybridKey.__init__).parameters
    assert "n_special" in inspect.signature(rns_ntt.RnsHybridKey.from_channels).parameters
    assert callable(rns_ntt.RnsHybridKey.restrict)  # stays
