"""Host-side checks of the NVFP4 folds (fa_fedavg_nvfp4, fa_fedavg_nvfp4_ptrs):
the symbols, their signatures beside fa_fedavg_mx's, the constants, and the
argument errors that are answered before anything touches a GPU."""
import ctypes

from fedlesscan_amd import _lib

NEW = {"fa_fedavg_nvfp4": "fa_fedavg_mx", "fa_fedavg_nvfp4_ptrs": "fa_fedavg_mx_ptrs"}


def test_entries_are_new_symbols_of_abi_7():
    L, B = _lib.load(), _lib.load_bench()
    assert L.fa_abi_version() == _lib.ABI_VERSION == 7
    assert set(NEW) <= set(_lib.header_functions())
    for name, parent in NEW.items():  # the MX entry's arguments without fmt
        assert hasattr(L, name) and _lib._PROTOS[name] == (_lib._PROTOS[parent][0], _lib._PROTOS[parent][1][1:])
    assert "fa_fedavg_nvfp4_form" in _lib.header_functions(_lib.BENCH_HEADER)
    assert hasattr(B, "fa_fedavg_nvfp4_form") and not hasattr(L, "fa_fedavg_nvfp4_form")
    header = open(_lib.HEADER).read()
    for name in ("FA_NVFP4_BLOCK", "FA_NVFP4_ROWS_AHEAD"):
        assert f"#define {name} {getattr(_lib, name)}\n" in header
    assert _lib.FA_NVFP4_BLOCK == 16


def test_argument_checks_answer_on_the_host():
    L = _lib.load()
    buf = (ctypes.c_uint8 * 1024)()
    p = (ctypes.addressof(buf) + 15) & ~15
    x, e, a, f32, b16 = p, p + 64, p + 128, p + 256, p + 512  # 2 rows of 32 columns (16 B, 2 scale bytes), outputs
    ARG = _lib.FA_ERR_ARG

    def fold(N=2, P=32, ldx=16, lde=2, out_f32=f32, out_bf16=None):
        return L.fa_fedavg_nvfp4(x, e, N, P, ldx, lde, a, None, None, 1.0, out_f32, out_bf16, None)

    assert fold(N=0) == _lib.FA_ERR_NO_CLIENTS
    assert fold(ldx=15) == _lib.FA_ERR_SHAPE and fold(lde=1) == _lib.FA_ERR_SHAPE
    assert fold(P=31, ldx=32) == ARG and "odd" in _lib.last_error()
    assert fold(out_f32=None) == ARG
    assert fold(out_f32=x + 28) == ARG and "fa_fedavg_nvfp4: an output overlaps" in _lib.last_error()
    assert fold(out_f32=e + 3) == ARG and fold(out_f32=None, out_bf16=e + 2) == ARG  # inside a scale row
    assert fold(out_f32=None, out_bf16=x + 16) == ARG
    assert fold(P=0) == _lib.FA_OK and fold(P=0, ldx=0, lde=0) == _lib.FA_OK  # nothing to fold
    # the row table: its own sizes, and the vector path's outputs
    def table(N=2, P=32, aligned=0, out_f32=f32, ei=e):
        return L.fa_fedavg_nvfp4_ptrs(x, ei, N, P, a, None, None, 1.0, aligned, out_f32, b16, None)

    assert table(N=0) == _lib.FA_ERR_NO_CLIENTS and table(P=31) == ARG and table(ei=None) == ARG
    assert table(aligned=1, out_f32=f32 + 4) == ARG and "aligned" in _lib.last_error()
    assert table(P=0) == _lib.FA_OK
    B = _lib.load_bench()
    assert B.fa_fedavg_nvfp4_form(x, e, 2, 32, 16, 2, a, None, None, 1.0, f32, None, None, 4, 2) == ARG
    assert B.fa_fedavg_nvfp4_form(x, e + 1, 2, 32, 16, 2, a, None, None, 1.0, f32, None, None, 3, 2) == ARG
