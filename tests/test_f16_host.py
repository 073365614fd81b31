"""CPU-side tests of the float16 fold's host pieces: the C-ABI entry and its
argument checks, the binary16 rounding of the factors, and the result dtype
numpy gives float16 layers.  No GPU compute (tests/test_gpu_f16.py has it)."""
import ctypes
import warnings

import numpy as np
import pytest

from fedlesscan_amd import _lib, engine


def test_library_exports_fa_fedavg_f16():
    L = _lib.load()
    assert "fa_fedavg_f16" in _lib.header_functions()
    assert hasattr(L, "fa_fedavg_f16")
    assert L.fa_abi_version() == _lib.ABI_VERSION == 7
    B = _lib.load_bench()
    n = B.fa_num_f16_forms()
    names = [B.fa_f16_form_name(i).decode() for i in range(n)]
    assert n >= 1 and all(nm.startswith("f16_") for nm in names) and len(set(names)) == n
    assert B.fa_f16_form_name(n) == b"" and B.fa_f16_form_name(-1) == b""
    # no name shared with the bf16 forms: the tuner's records hold forms by name
    assert not set(names) & {B.fa_bf16_form_name(i).decode() for i in range(B.fa_num_bf16_forms())}


def test_f16_argument_checks_equal_f32():
    """N == 0, ldx < P and a NULL out are refused before anything touches the
    GPU, with the status codes of fa_fedavg_f32."""
    L = _lib.load()
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.addressof(buf)
    one = 0x3C00  # 1.0
    cases = [
        dict(N=0, P=8, ldx=8, out=p),    # no clients
        dict(N=2, P=8, ldx=4, out=p),    # row pitch below the row length
        dict(N=2, P=8, ldx=8, out=None),  # NULL out
        dict(N=-1, P=8, ldx=8, out=p),
        dict(N=2, P=-3, ldx=8, out=p),
    ]
    for c in cases:
        rc16 = L.fa_fedavg_f16(p, c["N"], c["P"], c["ldx"], p, None, one, c["out"], None)
        msg16 = _lib.last_error()
        rc32 = L.fa_fedavg_f32(p, c["N"], c["P"], c["ldx"], p, None, 1.0, c["out"], None)
        assert rc16 == rc32 != _lib.FA_OK, c
        assert msg16 == _lib.last_error(), c
    assert L.fa_fedavg_f16(p, 0, 8, 8, p, None, one, p, None) == _lib.FA_ERR_NO_CLIENTS
    assert L.fa_fedavg_f16(p, 2, 8, 4, p, None, one, p, None) == _lib.FA_ERR_SHAPE
    assert L.fa_fedavg_f16(p, 2, 8, 8, p, None, one, None, None) == _lib.FA_ERR_ARG
    with pytest.raises(_lib.InvalidParameterShapeError):
        _lib.check(L.fa_fedavg_f16(p, 2, 8, 4, p, None, one, p, None), "fa_fedavg_f16")
    # the bench entry: the same checks, and an unknown form
    B = _lib.load_bench()
    assert B.fa_fedavg_f16_form(p, 0, 8, 8, p, None, one, p, None, 0) == _lib.FA_ERR_NO_CLIENTS
    assert B.fa_fedavg_f16_form(p, 2, 8, 4, p, None, one, p, None, 0) == _lib.FA_ERR_SHAPE
    assert B.fa_fedavg_f16_form(p, 2, 8, 8, p, None, one, p, None, B.fa_num_f16_forms()) == _lib.FA_ERR_ARG


_VALUES = [1, 3, 40, 2047, 2049, 4097, 65504, 65519, 65520, 70000, 0, -7, True,
           0.1, 1 / 3, 6.1e-5, 6e-8, 2.9e-8, 3e-8, 1e-9, 0.5, 1024.5, 65504.0, 65519.99, 65520.0, 7e4, -7e4,
           float("inf"), 2 ** 60, 2 ** 53 + 1]


def test_factors_round_once_to_binary16():
    """Factors(..., np.float16) == [np.float16(v) for v in ...]: one rounding of
    the Python number to half (2049 -> 2048, 65520 and 70000 -> inf), the total
    an exact Python sum rounded once."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # overflow in cast: inf, as in the reference
        exp = np.array([np.float16(v) for v in _VALUES], dtype=np.float16)
        f = engine.Factors(_VALUES, _VALUES, np.float16)
        assert f.a.dtype == np.float16 and f.s.dtype == np.float16
        assert np.array_equal(f.a.view(np.uint16), exp.view(np.uint16))
        assert np.array_equal(f.s.view(np.uint16), exp.view(np.uint16))
        assert np.float16(2049) == 2048 and np.isinf(np.float16(65520)) and np.isinf(np.float16(70000))
        for w in ([1, 2, 3], [2049], [30000, 30000, 5519], [30000, 30000, 5520], [40000, 40000], [0.1, 0.2]):
            f = engine.Factors(w, None, np.float16)
            assert f.s is None and type(f.div) is np.float16
            assert f.div.view(np.uint16) == np.float16(sum(w)).view(np.uint16), w
        f = engine.Factors([1, 2], None, np.float16, total=2049)
        assert f.div == np.float16(2048)
        # scores are Python floats from a double division, rounded once to half
        sc = [(r + 1) / 11 for r in range(11)]
        f = engine.Factors([1] * 11, sc, np.float16)
        assert np.array_equal(f.s.view(np.uint16), np.array([np.float16(x) for x in sc]).view(np.uint16))


def test_result_dtype_of_float16_rows():
    f16 = np.dtype(np.float16)
    assert engine.result_dtype(f16, [1, 2, 3]) == np.float16
    assert engine.result_dtype(f16, [1, 2.5, True], [0.5, 1.0, 1.0]) == np.float16
    assert engine.result_dtype(f16, [70000, 1]) == np.float16
    assert engine.result_dtype(f16, [1, 2], None, total=10) == np.float16
    assert engine.result_dtype(f16, [np.float32(1), 2]) == np.float32
    assert engine.result_dtype(f16, [1, 2], [np.float32(0.5), 1.0]) == np.float32
    assert engine.result_dtype(f16, [np.float64(1), 2]) == np.float64
    assert engine.result_dtype(f16, [np.int64(3), np.int64(4)]) == np.float64
    # what numpy itself gives
    x = np.ones(3, np.float16)
    assert (x * 3 / 5).dtype == np.float16
    assert (x * np.float32(3)).dtype == np.float32
    assert (x * np.int64(3)).dtype == np.float64
    import torch
    assert engine._NP_TO_TORCH[f16] == torch.float16
