"""Host-side checks of the quantising folds (fa_fedavg_mx_q, fa_fedavg_fp8_q and
their _ptrs entries): the symbols, their signatures beside their parents', and
the argument errors that are answered before anything touches a GPU."""
import ctypes

from fedlesscan_amd import _lib

NEW = {"fa_fedavg_mx_q": "fa_fedavg_mx", "fa_fedavg_mx_q_ptrs": "fa_fedavg_mx_ptrs",
       "fa_fedavg_fp8_q": "fa_fedavg_fp8", "fa_fedavg_fp8_q_ptrs": "fa_fedavg_fp8_ptrs"}


def test_entries_are_new_symbols_of_abi_7():
    L, B = _lib.load(), _lib.load_bench()
    assert L.fa_abi_version() == _lib.ABI_VERSION == 7
    assert set(NEW) <= set(_lib.header_functions())
    assert "fa_fedavg_mx_q_form" in _lib.header_functions(_lib.BENCH_HEADER)
    assert hasattr(B, "fa_fedavg_mx_q_form") and not hasattr(L, "fa_fedavg_mx_q_form")
    for q, parent in NEW.items():  # out_bf16 gives way to out_fmt, out_q, out_e
        (_, pa), (_, qa) = _lib._PROTOS[parent], _lib._PROTOS[q]
        assert qa == pa[:-2] + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p] + pa[-1:]
    header = open(_lib.HEADER).read()
    for name, value in (("FA_MX_E4M3", 0), ("FA_MX_E5M2", 1), ("FA_MX_E2M1", 2)):
        assert f"#define {name} {value}" in header and getattr(_lib, name) == value


def test_argument_checks_answer_on_the_host():
    L = _lib.load()
    buf = (ctypes.c_uint8 * 1024)()
    p = (ctypes.addressof(buf) + 15) & ~15
    x, e, a, f32, q, oe = p, p + 128, p + 192, p + 256, p + 512, p + 640  # 2 rows of 32 columns and their outputs
    ARG = _lib.FA_ERR_ARG

    def mx(fmt=0, N=2, P=32, out_f32=f32, out_fmt=0, out_q=q, out_e=oe, ldx=32):
        return L.fa_fedavg_mx_q(fmt, x, e, N, P, ldx, 1, a, None, None, 1.0, out_f32, out_fmt, out_q, out_e, None)

    def fp8(N=2, P=32, out_f32=f32, out_fmt=0, out_q=q, out_e=oe, ldx=32):
        return L.fa_fedavg_fp8_q(0, x, N, P, ldx, a, None, None, 1.0, out_f32, out_fmt, out_q, out_e, None)

    for fold in (mx, fp8):
        assert fold(N=0) == _lib.FA_ERR_NO_CLIENTS
        assert fold(ldx=16) == _lib.FA_ERR_SHAPE
        assert fold(out_fmt=3) == ARG and "format" in _lib.last_error()
        assert fold(out_fmt=_lib.FA_MX_E2M1, P=31) == ARG and "odd" in _lib.last_error()
        assert fold(out_q=None) == ARG and fold(out_e=None) == ARG
        assert fold(out_q=x + 40) == ARG and "overlaps" in _lib.last_error()  # the codes in a row
        assert fold(out_f32=x) == ARG and fold(out_e=x + 63) == ARG
        assert fold(out_e=q + 31) == ARG and "one another" in _lib.last_error()
        assert fold(out_f32=q - 124) == ARG and fold(out_f32=oe - 127) == ARG
        assert fold(P=0) == _lib.FA_OK  # nothing to fold
    assert mx(out_e=e + 1) == ARG and mx(out_q=e - 31) == ARG  # an output in the rows' scale bytes
    assert mx(fmt=3) == ARG
    # the row tables: the outputs' own checks, and the vector path's alignment
    assert L.fa_fedavg_mx_q_ptrs(0, x, e, 2, 32, a, None, None, 1.0, 1, f32, 3, q, oe, None) == ARG
    assert L.fa_fedavg_mx_q_ptrs(0, x, e, 2, 32, a, None, None, 1.0, 1, f32, 0, q + 4, oe, None) == ARG
    assert L.fa_fedavg_mx_q_ptrs(0, x, e, 2, 32, a, None, None, 1.0, 0, f32, 0, q, q + 8, None) == ARG
    assert L.fa_fedavg_fp8_q_ptrs(0, x, 2, 31, a, None, None, 1.0, 0, f32, 2, q, oe, None) == ARG
    assert L.fa_fedavg_fp8_q_ptrs(0, x, 2, 32, a, None, None, 1.0, 1, f32 + 4, 0, q, oe, None) == ARG
    assert L.fa_fedavg_fp8_q_ptrs(2, x, 2, 32, a, None, None, 1.0, 0, f32, 0, q, oe, None) == ARG
    B = _lib.load_bench()
    assert B.fa_fedavg_mx_q_form(0, x, e, 2, 32, 32, 1, a, 1.0, f32, 0, q, oe, None, 5) == ARG
    assert B.fa_fedavg_mx_q_form(0, x, e, 2, 32, 32, 1, a, 1.0, f32, 0, q + 1, oe, None, 0) == ARG
