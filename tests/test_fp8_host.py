"""Host-side checks of the fp8 folds: the entries, argument checks that answer
before anything touches the GPU, ScaledLayer unwrapping."""
import ctypes

import pytest

from fedlesscan_amd import _lib


def test_entries_are_new_symbols_of_abi_7():
    L, B = _lib.load(), _lib.load_bench()
    assert L.fa_abi_version() == _lib.ABI_VERSION == 7
    assert {"fa_fedavg_fp8", "fa_fedavg_fp8_ptrs"} <= set(_lib.header_functions())
    assert hasattr(B, "fa_fedavg_fp8_form") and not hasattr(L, "fa_fedavg_fp8_form")


def test_argument_checks_answer_on_the_host():
    L = _lib.load()
    buf = (ctypes.c_uint8 * 256)()
    p = (ctypes.addressof(buf) + 15) & ~15
    for fmt in (_lib.FA_FP8_E4M3FN, _lib.FA_FP8_E5M2):
        assert L.fa_fedavg_fp8(fmt, p, 0, 16, 16, p, None, None, 1.0, p, None, None) == _lib.FA_ERR_NO_CLIENTS
        assert L.fa_fedavg_fp8(fmt, p, 2, 16, 8, p, None, None, 1.0, p, None, None) == _lib.FA_ERR_SHAPE
        assert L.fa_fedavg_fp8(fmt, p, 2, 16, 16, p, None, None, 1.0, None, None, None) == _lib.FA_ERR_ARG  # no output
        assert L.fa_fedavg_fp8(fmt, p, 2, 16, 16, p, None, None, 1.0, p + 16, None, None) == _lib.FA_ERR_ARG
        assert "overlaps" in _lib.last_error()
        assert L.fa_fedavg_fp8(fmt, p, 2, 0, 0, p, None, None, 1.0, p, None, None) == _lib.FA_OK  # P == 0: nothing
        assert L.fa_fedavg_fp8_ptrs(fmt, p, 0, 16, p, None, None, 1.0, 1, p, None, None) == _lib.FA_ERR_NO_CLIENTS
        assert L.fa_fedavg_fp8_ptrs(fmt, None, 2, 16, p, None, None, 1.0, 0, p, None, None) == _lib.FA_ERR_ARG
        assert L.fa_fedavg_fp8_ptrs(fmt, p, 2, 16, p, None, None, 1.0, 1, p + 4, None, None) == _lib.FA_ERR_ARG
    assert L.fa_fedavg_fp8(2, p, 2, 16, 16, p, None, None, 1.0, p + 64, None, None) == _lib.FA_ERR_ARG
    assert "format" in _lib.last_error()
    assert L.fa_fedavg_fp8_ptrs(-1, p, 2, 16, p, None, None, 1.0, 0, p, None, None) == _lib.FA_ERR_ARG
    # the bench entry: forms 0..3 over at least one block per CU, the vector path only
    B = _lib.load_bench()
    assert B.fa_fedavg_fp8_form(p, 2, 16, 16, p, None, None, 1.0, p + 64, None, None, 4, 1) == _lib.FA_ERR_ARG
    assert B.fa_fedavg_fp8_form(p, 2, 16, 16, p, None, None, 1.0, p + 64, None, None, 3, 0) == _lib.FA_ERR_ARG
    assert B.fa_fedavg_fp8_form(p + 1, 2, 16, 16, p, None, None, 1.0, p + 64, None, None, 3, 1) == _lib.FA_ERR_ARG


def test_scaled_layers_unwrap_all_or_none():
    torch = pytest.importorskip("torch")
    from fedlesscan_amd import InvalidParameterShapeError, ScaledLayer, engine
    q = torch.zeros(4, dtype=torch.uint8).view(torch.float8_e5m2)
    f = torch.zeros(4)
    plain, scales = engine._unwrap_scaled([[f, ScaledLayer(q, 0.5)], [f, ScaledLayer(q, 2.0)], [f]], 2)
    assert scales == {1: [0.5, 2.0]} and all(p[1] is q and p[0] is f for p in plain) and len(plain) == 2
    same = [[f, q], [f, q]]
    assert engine._unwrap_scaled(same, 2) == (same, {})
    with pytest.raises(InvalidParameterShapeError, match="layer 1"):
        engine._unwrap_scaled([[f, ScaledLayer(q, 0.5)], [f, q]], 2)
    with pytest.raises(InvalidParameterShapeError, match="fp8"):  # a scale on rows that are not fp8
        engine.aggregate_layers([[ScaledLayer(f, 0.5)], [ScaledLayer(f, 2.0)]], [1, 2])
