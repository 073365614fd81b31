"""CPU-side tests of the 16-bit row-table folds' host pieces: the three product
entries and the bench-library entries exist with the declared signatures, the
ABI number stays 7, the argument checks answer before anything touches the
GPU, and RowSet's placement arithmetic uses the rows' element size.  No GPU
compute (tests/test_gpu_rows16.py has it)."""
import ctypes
import re

import numpy as np

from fedlesscan_amd import _lib, engine

PRODUCT = {
    "fa_fedavg_bf16_ptrs": (
        "int", ["const uint16_t* const*", "int64_t", "int64_t", "const float*", "const float*", "float", "int",
                "float*", "uint16_t*", "void*"]),
    "fa_fedavg_bf16_ptrs_hostf": (
        "int", ["const uint16_t* const*", "int64_t", "int64_t", "const float*", "const float*", "float", "int",
                "float*", "uint16_t*", "void*"]),
    "fa_fedavg_f16_ptrs": (
        "int", ["const uint16_t* const*", "int64_t", "int64_t", "const uint16_t*", "const uint16_t*", "uint16_t",
                "int", "uint16_t*", "void*"]),
}
BENCH = {
    "fa_num_rows16_forms": ("int", ["void"]),
    "fa_rows16_form_name": ("const char*", ["int"]),
    "fa_fedavg_bf16_ptrs_form": ("int", PRODUCT["fa_fedavg_bf16_ptrs"][1] + ["int"]),
    "fa_fedavg_f16_ptrs_form": ("int", PRODUCT["fa_fedavg_f16_ptrs"][1] + ["int"]),
}
_CTYPE = {"int64_t": ctypes.c_int64, "float": ctypes.c_float, "int": ctypes.c_int, "uint16_t": ctypes.c_uint16}


def _declaration(header: str, name: str):
    """(return type, [parameter types]) of `name` as the header declares it."""
    with open(header) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"([A-Za-z_][\w \*]*?)\b" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in {header}"

    def norm(t):  # one spelling per type: "const uint16_t* const*"
        return re.sub(r"\s*\*\s*", "* ", " ".join(t.split())).strip()

    params = []
    for p in m.group(2).split(","):
        p = norm(p)
        params.append(p if p == "void" else norm(re.sub(r"\b\w+$", "", p)))  # without the parameter's name
    return norm(m.group(1)), params


def _ctypes_of(params):
    return [] if params == ["void"] else [ctypes.c_void_p if p.endswith("*") else _CTYPE[p] for p in params]


def test_product_entries_exist_with_the_declared_signatures():
    L = _lib.load()
    assert L.fa_abi_version() == _lib.ABI_VERSION == 7  # new symbols only
    declared = _lib.header_functions()
    for name, (ret, params) in PRODUCT.items():
        assert name in declared and hasattr(L, name), name
        assert _declaration(_lib.HEADER, name) == (ret, params), name
        res, args = _lib._PROTOS[name]
        assert res is ctypes.c_int and args == _ctypes_of(params), name


def test_bench_entries_exist_with_the_declared_signatures():
    L, B = _lib.load(), _lib.load_bench()
    declared = _lib.header_functions(_lib.BENCH_HEADER)
    for name, (ret, params) in BENCH.items():
        assert name in declared and hasattr(B, name) and not hasattr(L, name), name
        assert _declaration(_lib.BENCH_HEADER, name) == (ret, params), name
        res, args = _lib._BENCH_PROTOS[name]
        assert res is (ctypes.c_char_p if ret == "const char*" else ctypes.c_int) and args == _ctypes_of(params), name


def test_form_names_distinct_and_non_empty():
    B = _lib.load_bench()
    n = B.fa_num_rows16_forms()
    names = [B.fa_rows16_form_name(i).decode() for i in range(n)]
    assert n >= 5 and all(names) and len(set(names)) == n, names  # four octet forms and the column form
    assert B.fa_rows16_form_name(n) == b"" and B.fa_rows16_form_name(-1) == b""
    # forms travel by name: none shared with the stacked 16-bit folds or the fp32 row table
    other = {B.fa_bf16_form_name(i).decode() for i in range(B.fa_num_bf16_forms())}
    other |= {B.fa_f16_form_name(i).decode() for i in range(B.fa_num_f16_forms())}
    other |= {B.fa_ptrs_form_name(i).decode() for i in range(B.fa_num_ptrs_forms())}
    assert not set(names) & other


def test_argument_checks_answer_on_the_host():
    """N == 0, negative sizes and NULL pointers are refused before anything
    touches the GPU, with the codes of fa_fedavg_f32_ptrs / fa_fedavg_bf16 /
    fa_fedavg_f16; the _hostf entry reports the same."""
    L, B = _lib.load(), _lib.load_bench()
    buf = (ctypes.c_uint8 * 256)()
    p = (ctypes.addressof(buf) + 15) & ~15  # 16-B aligned, so p + 2 and p + 4 are not
    one = 0x3C00  # 1.0 in binary16
    for aligned in (0, 1):
        assert L.fa_fedavg_bf16_ptrs(p, 0, 8, p, None, 1.0, aligned, p, None, None) == _lib.FA_ERR_NO_CLIENTS
        assert L.fa_fedavg_bf16_ptrs(p, 2, 8, p, None, 1.0, aligned, None, None, None) == _lib.FA_ERR_ARG  # no output
        assert "null" in _lib.last_error()
        assert L.fa_fedavg_bf16_ptrs(None, 2, 8, p, None, 1.0, aligned, p, p, None) == _lib.FA_ERR_ARG
        assert L.fa_fedavg_bf16_ptrs(p, 2, 8, None, None, 1.0, aligned, p, p, None) == _lib.FA_ERR_ARG
        assert L.fa_fedavg_bf16_ptrs(p, -1, 8, p, None, 1.0, aligned, p, p, None) == _lib.FA_ERR_ARG
        assert L.fa_fedavg_bf16_ptrs(p, 2, -8, p, None, 1.0, aligned, p, p, None) == _lib.FA_ERR_ARG
        assert L.fa_fedavg_bf16_ptrs_hostf(p, 0, 8, p, None, 1.0, aligned, p, None, None) == _lib.FA_ERR_NO_CLIENTS
        assert L.fa_fedavg_bf16_ptrs_hostf(p, -1, 8, p, None, 1.0, aligned, p, None, None) == _lib.FA_ERR_ARG
        assert L.fa_fedavg_f16_ptrs(p, 0, 8, p, None, one, aligned, p, None) == _lib.FA_ERR_NO_CLIENTS
        assert L.fa_fedavg_f16_ptrs(p, 2, 8, p, None, one, aligned, None, None) == _lib.FA_ERR_ARG
        assert L.fa_fedavg_f16_ptrs(None, 2, 8, p, None, one, aligned, p, None) == _lib.FA_ERR_ARG
        assert L.fa_fedavg_f16_ptrs(p, 2, -8, p, None, one, aligned, p, None) == _lib.FA_ERR_ARG
        # the same message as the stacked folds give for the same mistake
        L.fa_fedavg_bf16_ptrs(p, 0, 8, p, None, 1.0, aligned, p, None, None)
        msg = _lib.last_error()
        L.fa_fedavg_bf16(p, 0, 8, 8, p, None, 1.0, p, None, None)
        assert msg == _lib.last_error()
    # rows promised aligned, an output that is not: refused, nothing launched
    assert L.fa_fedavg_bf16_ptrs(p, 2, 8, p, None, 1.0, 1, p + 4, None, None) == _lib.FA_ERR_ARG
    assert L.fa_fedavg_bf16_ptrs(p, 2, 8, p, None, 1.0, 1, p, p + 2, None) == _lib.FA_ERR_ARG
    assert L.fa_fedavg_f16_ptrs(p, 2, 8, p, None, one, 1, p + 2, None) == _lib.FA_ERR_ARG
    # the bench entries: the same checks, an unknown form, an octet form without the promise
    n = B.fa_num_rows16_forms()
    assert B.fa_fedavg_bf16_ptrs_form(p, 0, 8, p, None, 1.0, 1, p, None, None, 0) == _lib.FA_ERR_NO_CLIENTS
    assert B.fa_fedavg_bf16_ptrs_form(p, 2, 8, p, None, 1.0, 1, None, None, None, -1) == _lib.FA_ERR_ARG
    assert B.fa_fedavg_bf16_ptrs_form(p, 2, 8, p, None, 1.0, 1, p, None, None, n) == _lib.FA_ERR_ARG
    assert B.fa_fedavg_bf16_ptrs_form(p, 2, 8, p, None, 1.0, 0, p, None, None, 0) == _lib.FA_ERR_ARG
    assert B.fa_fedavg_f16_ptrs_form(p, 0, 8, p, None, one, 1, p, None, 0) == _lib.FA_ERR_NO_CLIENTS
    assert B.fa_fedavg_f16_ptrs_form(p, 2, 8, p, None, one, 1, p, None, n) == _lib.FA_ERR_ARG
    assert B.fa_fedavg_f16_ptrs_form(p, 2, 8, p, None, one, 0, p, None, 0) == _lib.FA_ERR_ARG


class _Row:
    """What RowSet's placement arithmetic asks of a row, without a GPU."""

    def __init__(self, ptr, esize, storage=0):
        self.ptr, self.esize, self.storage = ptr, esize, storage

    def element_size(self):
        return self.esize

    def untyped_storage(self):
        return self

    def data_ptr(self):
        return self.storage

    def as_strided(self, size, stride):
        return size, stride


def test_equal_stride_view_uses_the_element_size():
    """A constant pitch counts in elements of the rows' dtype: 2-byte rows at a
    pitch of P * 2 + 2 bytes are a view (pitch P + 1), at an odd byte pitch or a
    pitch below the row length they are not; 4-byte rows as before."""
    P = 5

    def view(esize, step, n=3):
        rows = [_Row(1000 + i * step, esize) for i in range(n)]
        return engine._equal_stride_view(rows, np.array([r.ptr for r in rows], np.int64), P)

    assert view(2, P * 2) == ((3, P), (P, 1))
    assert view(2, P * 2 + 2) == ((3, P), (P + 1, 1))
    assert view(2, P * 2 + 6) == ((3, P), (P + 3, 1))  # 16 bytes: no multiple of 4 elements needed
    assert view(2, P * 2 + 1) is None and view(2, P * 2 - 2) is None and view(2, -P * 2) is None
    assert view(4, P * 4) == ((3, P), (P, 1)) and view(4, P * 4 + 4) == ((3, P), (P + 1, 1))
    assert view(4, P * 4 + 2) is None and view(4, P * 2) is None
    assert engine.stats.keys() >= {"rows16_folds", "stacked_groups"}
