"""Host-side checks of the MX layer tables (fa_fedavg_mx_layers,
fa_fedavg_mx_q_layers): the wave-tile planner fa_mx_layers_plan against the
header's formulas, and the argument errors of the two entries and of their
bench forms, answered before anything touches a GPU (tests/test_gpu_mx_layers.py
has the compute)."""
import ctypes

from fedlesscan_amd import _lib, engine


def test_wave_tile_plan():
    cols, al = [0, 30, 32, 2048, 2049, 5 * 2048 + 96 + 6, 64], [1, 1, 1, 1, 1, 0, 1]
    plan, tiles, elems = engine.mx_layer_plan(cols, al)
    # ceil(ceil(cols / 32) / 64) wave tiles, the unaligned layer ceil(cols / 64), none for 0 columns
    ceil = lambda n, d: -(-n // d)
    per = [ceil(ceil(n, 32), 64) if a else ceil(n, 64) for n, a in zip(cols, al)]
    assert per == [0, 1, 1, 1, 2, 162, 1]
    assert plan[:, 0].tolist() == cols and plan[:, 3].tolist() == al
    assert plan[:, 2].tolist() == [sum(per[:k]) for k in range(len(cols))] and tiles == sum(per)
    offs = [sum(-(-n // 64) * 64 for n in cols[:k]) for k in range(len(cols) + 1)]
    assert plan[:, 1].tolist() == offs[:-1] and elems == offs[-1]
    assert engine.mx_layer_plan([], [])[1:] == (0, 0)
    L = _lib.load()
    c, a = (ctypes.c_int64 * 1)(-1), (ctypes.c_int32 * 1)(1)
    p, t, e = (ctypes.c_int64 * 4)(), ctypes.c_int64(), ctypes.c_int64()
    ad = ctypes.addressof
    assert L.fa_mx_layers_plan(ad(c), ad(a), 1, ad(p), ad(t), ad(e)) == _lib.FA_ERR_ARG  # a negative column count
    assert L.fa_mx_layers_plan(ad(c), ad(a), -1, ad(p), ad(t), ad(e)) == _lib.FA_ERR_ARG
    assert L.fa_mx_layers_plan(ad(c), ad(a), 1, None, ad(t), ad(e)) == _lib.FA_ERR_ARG


def test_argument_checks_answer_on_the_host():
    L, B = _lib.load(), _lib.load_bench()
    assert L.fa_abi_version() == _lib.ABI_VERSION == 7  # new symbols only
    assert {"fa_mx_layers_plan", "fa_fedavg_mx_layers", "fa_fedavg_mx_q_layers"} <= set(_lib.header_functions())
    assert f"#define FA_MX_WAVE_TILE_COLS {_lib.FA_MX_WAVE_TILE_COLS}" in open(_lib.HEADER).read()
    assert "mx_table_folds" in engine.stats
    buf = (ctypes.c_uint8 * 1024)()
    p = (ctypes.addressof(buf) + 15) & ~15
    xi, ei, plan, a, f32, q, oe = p, p + 64, p + 128, p + 192, p + 256, p + 512, p + 640
    ARG = _lib.FA_ERR_ARG

    def plain(cap=None, fmt=0, xi=xi, ei=ei, plan=plan, L_=1, N=2, tiles=1, a=a, out=f32, outb=None):
        args = (fmt, xi, ei, plan, L_, N, tiles, a, None, None, 1.0, out, outb, None)
        return L.fa_fedavg_mx_layers(*args) if cap is None else B.fa_fedavg_mx_layers_form(*args, cap)

    def quant(cap=None, fmt=0, xi=xi, ei=ei, plan=plan, L_=1, N=2, tiles=1, a=a, out=f32, out_fmt=0, out_q=q, out_e=oe):
        args = (fmt, xi, ei, plan, L_, N, tiles, a, None, None, 1.0, out, out_fmt, out_q, out_e, None)
        return L.fa_fedavg_mx_q_layers(*args) if cap is None else B.fa_fedavg_mx_q_layers_form(*args, cap)

    for fold, cap in ((plain, None), (quant, None), (plain, 3), (quant, 3)):
        assert fold(cap, fmt=3) == ARG
        assert fold(cap, L_=-1) == ARG and fold(cap, N=-1) == ARG and fold(cap, tiles=-1) == ARG
        assert fold(cap, N=0) == _lib.FA_ERR_NO_CLIENTS
        assert fold(cap, xi=None) == ARG and fold(cap, ei=None) == ARG and fold(cap, plan=None) == ARG
        assert fold(cap, a=None) == ARG
        assert fold(cap, out=f32 + 4) == ARG and "16-B aligned" in (
            _lib.load_bench().fa_bench_last_error().decode() if cap else _lib.last_error())
        assert fold(cap, L_=0) == _lib.FA_OK and fold(cap, tiles=0) == _lib.FA_OK  # nothing to fold
    assert plain(out=None) == ARG and plain(out=None, outb=f32 + 2) == ARG
    assert quant(out_fmt=3) == ARG and quant(out_q=None) == ARG and quant(out_e=None) == ARG
    assert quant(out_q=q + 1) == ARG
    assert plain(-1) == ARG and quant(-1) == ARG  # a negative grid cap
