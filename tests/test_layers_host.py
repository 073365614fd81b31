"""CPU-side tests of the layer-table folds' host pieces (fa_fedavg_*_layers):
the host planner fa_layers_plan against its rule restated here, the argument
checks of the four entries and of the bench library's form entry, and the new
symbols.  No GPU compute (tests/test_gpu_layers.py has it)."""
import ctypes

import numpy as np
import pytest

from fedlesscan_amd import _lib, engine

BLOCK = 256
ENTRIES = ["fa_fedavg_f32_layers", "fa_fedavg_bf16_layers", "fa_fedavg_f16_layers", "fa_fedavg_f64_layers"]


def _tiles(cols, aligned, units, lg):
    """The tiles of one layer, as include/fedavg_hip.h states them."""
    if cols == 0:
        return 0
    if not aligned:
        return -(-cols // BLOCK)
    u = (cols >> lg) + (1 if cols & ((1 << lg) - 1) else 0)
    return -(-u // (BLOCK * units))


def _grid(tiles, cus):
    """At most one block per CU, balanced passes."""
    if tiles == 0:
        return 0
    g = min(cus, tiles)
    passes = -(-tiles // g)
    return -(-tiles // passes)


def _rule(cols, aligned, lg, cus):
    for c in (4, 2):
        if _grid(sum(_tiles(n, al, c, lg) for n, al in zip(cols, aligned)), cus) * 8 >= cus * 7:
            return c
    return 1


def _expected(cols, aligned, lg, units):
    plan, t, off = [], 0, 0
    for n, al in zip(cols, aligned):
        plan.append((n, off, t, int(bool(al))))
        t += _tiles(n, al, units, lg)
        off += -(-n // 64) * 64
    return np.array(plan, dtype=np.int64).reshape(len(cols), 4), t, off


def test_new_symbols_are_declared_and_exported():
    L = _lib.load()
    assert L.fa_abi_version() == _lib.ABI_VERSION == 7  # new symbols only
    declared = _lib.header_functions()
    for name in ENTRIES + ["fa_layers_plan"]:
        assert name in declared and name in _lib._PROTOS and hasattr(L, name), name
    B = _lib.load_bench()
    assert "fa_fedavg_layers_form" in _lib.header_functions(_lib.BENCH_HEADER)
    assert "fa_fedavg_layers_form" in _lib._BENCH_PROTOS and hasattr(B, "fa_fedavg_layers_form")
    assert not hasattr(L, "fa_fedavg_layers_form")
    assert "layer_table_folds" in engine.stats


@pytest.mark.parametrize("lg", [1, 2, 3])
def test_plan_of_the_parity_model(lg):
    """A zero-width layer, a layer that ends exactly on a tile boundary, a
    layer of one column, layers with P % unit != 0."""
    u = 1 << lg
    cols = [u * 256 * 4 + 13, 5, 0, u * 256, 1, u * 256 * 2 + u]
    al = [True] * len(cols)
    plan, tiles, elems, units = engine.layer_plan(cols, al, lg, cus=256, units=1)
    assert units == 1
    # units: 1024 + the tail lane's, 1 (tail only), 0, exactly 256, 1, 513
    assert plan[:, 2].tolist() == [0, 5, 6, 6, 7, 8] and tiles == 11
    assert plan[:, 0].tolist() == cols and plan[:, 3].tolist() == [1] * 6
    plan4, tiles4, _, units4 = engine.layer_plan(cols, al, lg, cus=256, units=4)
    assert units4 == 4 and plan4[:, 2].tolist() == [0, 2, 3, 3, 4, 5] and tiles4 == 6
    for un in (1, 2, 4):
        p, t, e, _ = engine.layer_plan(cols, al, lg, cus=256, units=un)
        ep, et, ee = _expected(cols, al, lg, un)
        assert np.array_equal(p, ep) and t == et and e == ee
    # output offsets: multiples of 64 elements, in order, not overlapping
    off = plan[:, 1]
    assert not (off % 64).any() and off[0] == 0
    assert all(off[k + 1] >= off[k] + cols[k] for k in range(len(cols) - 1))
    assert elems >= off[-1] + cols[-1] and elems % 64 == 0


def test_plan_unaligned_layer_between_aligned_ones():
    cols, al = [8 * 256, 300, 8 * 256 + 3], [True, False, True]
    plan, tiles, elems, _ = engine.layer_plan(cols, al, 3, cus=256, units=2)
    # one tile of 2 octets per lane; one column per lane: ceil(300 / 256); 256 octets + the tail lane's
    assert plan[:, 2].tolist() == [0, 1, 3] and tiles == 4
    assert plan[:, 3].tolist() == [1, 0, 1]
    assert plan[:, 1].tolist() == [0, 2048, 2048 + 320] and elems == 2048 + 320 + 2112
    # an unaligned layer's tiles do not depend on the units per lane
    for un in (1, 4):
        p, _, _, _ = engine.layer_plan(cols, al, 3, cus=256, units=un)
        assert p[2, 2] - p[1, 2] == 2


def test_plan_empty_models():
    plan, tiles, elems, units = engine.layer_plan([], [], 2, cus=256)
    assert plan.shape == (0, 4) and tiles == 0 and elems == 0 and units == 1
    plan, tiles, elems, units = engine.layer_plan([0, 0], [True, True], 2, cus=256)
    assert tiles == 0 and elems == 0 and plan[:, 2].tolist() == [0, 0]


@pytest.mark.parametrize("lg", [1, 2, 3])
def test_units_rule_around_seven_eighths_of_the_cus(lg):
    """The most of 4, 2, 1 units per lane whose balanced grid over the model's
    total tiles covers 7/8 of the CUs, else 1: 64 CUs, layers of exactly one
    4-unit tile each."""
    cus, one4 = 64, (1 << lg) * 256 * 4
    # 55 tiles: one short of 7/8 x 64 = 56 blocks with 4 units, and two passes of 55 with 2; 65: two
    # passes of 33; 27 / 28 layers: 54 / 56 tiles with 2 units; 14: no width reaches 56 blocks
    for n, want in [(55, 1), (56, 4), (57, 4), (64, 4), (65, 1), (27, 1), (28, 2), (14, 1)]:
        cols, al = [one4] * n, [True] * n
        assert want == _rule(cols, al, lg, cus), n
        _, tiles, _, units = engine.layer_plan(cols, al, lg, cus)
        assert units == want, (n, units)
        assert tiles == n * (4 // units)
    # mixed models against the rule restated above
    rng = np.random.default_rng(5)
    for _ in range(50):
        n = int(rng.integers(1, 40))
        cols = [int(x) for x in rng.integers(0, 40000, n)]
        al = [bool(x) for x in rng.integers(0, 4, n)]
        cu = int(rng.choice([8, 64, 256]))
        p, t, e, units = engine.layer_plan(cols, al, lg, cu)
        assert units == _rule(cols, al, lg, cu)
        ep, et, ee = _expected(cols, al, lg, units)
        assert np.array_equal(p, ep) and t == et and e == ee


def test_planner_argument_checks():
    L = _lib.load()
    c = (ctypes.c_int64 * 2)(8, 8)
    al = (ctypes.c_int32 * 2)(1, 1)
    plan = (ctypes.c_int64 * 8)()
    t, e, u = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
    pc, pa, pp = (ctypes.addressof(x) for x in (c, al, plan))
    pt, pe, pu = (ctypes.addressof(x) for x in (t, e, u))
    assert L.fa_layers_plan(pc, pa, 2, 3, 256, 0, pp, pt, pe, pu) == _lib.FA_OK
    assert L.fa_layers_plan(pc, pa, -1, 3, 256, 0, pp, pt, pe, pu) == _lib.FA_ERR_ARG
    assert L.fa_layers_plan(pc, pa, 2, 0, 256, 0, pp, pt, pe, pu) == _lib.FA_ERR_ARG
    assert L.fa_layers_plan(pc, pa, 2, 4, 256, 0, pp, pt, pe, pu) == _lib.FA_ERR_ARG
    assert L.fa_layers_plan(pc, pa, 2, 3, 0, 0, pp, pt, pe, pu) == _lib.FA_ERR_ARG
    assert L.fa_layers_plan(pc, pa, 2, 3, 256, 3, pp, pt, pe, pu) == _lib.FA_ERR_ARG
    assert L.fa_layers_plan(None, pa, 2, 3, 256, 0, pp, pt, pe, pu) == _lib.FA_ERR_ARG
    assert L.fa_layers_plan(pc, pa, 2, 3, 256, 0, None, pt, pe, pu) == _lib.FA_ERR_ARG
    assert L.fa_layers_plan(pc, pa, 2, 3, 256, 0, pp, None, pe, pu) == _lib.FA_ERR_ARG
    c[1] = -4
    assert L.fa_layers_plan(pc, pa, 2, 3, 256, 0, pp, pt, pe, pu) == _lib.FA_ERR_ARG
    assert "layer 1" in _lib.last_error()


def _call(lib, name, p, *, L=2, N=2, tiles=3, units=1, out="p", xi="p", cap=0, dtype=None):
    """One of the four entries, or the form entry (dtype given), over host
    scratch: every case here is refused, or returns, before any launch."""
    o = p if out == "p" else out
    x = p if xi == "p" else xi
    if dtype is not None:
        return lib.fa_fedavg_layers_form(dtype, x, p, L, N, tiles, units, cap, p, None, 1.0, o, None, None)
    if name == "fa_fedavg_bf16_layers":
        return getattr(lib, name)(x, p, L, N, tiles, units, p, None, 1.0, o, None, None)
    if name == "fa_fedavg_f16_layers":
        return getattr(lib, name)(x, p, L, N, tiles, units, p, None, 0x3C00, o, None)
    return getattr(lib, name)(x, p, L, N, tiles, units, p, None, 1.0, o, None)


@pytest.mark.parametrize("name", ENTRIES + ["form"])
def test_layers_argument_checks(name):
    """Refused before anything touches the GPU, with the status codes of the
    row-table folds: no clients, negative sizes, units outside {1, 2, 4}, NULL
    pointers, an output off 16-B alignment; nothing to fold returns FA_OK."""
    form = name == "form"
    lib = _lib.load_bench() if form else _lib.load()
    buf = (ctypes.c_uint8 * 512)()
    p = (ctypes.addressof(buf) + 15) & ~15
    for dt in ([0, 1, 2, 3] if form else [None]):
        kw = dict(dtype=dt)
        assert _call(lib, name, p, N=0, **kw) == _lib.FA_ERR_NO_CLIENTS
        assert _call(lib, name, p, N=-1, **kw) == _lib.FA_ERR_ARG
        assert _call(lib, name, p, L=-1, **kw) == _lib.FA_ERR_ARG
        assert _call(lib, name, p, tiles=-1, **kw) == _lib.FA_ERR_ARG
        for units in (0, 3, 8, -1):
            assert _call(lib, name, p, units=units, **kw) == _lib.FA_ERR_ARG
        assert _call(lib, name, p, out=None, **kw) == _lib.FA_ERR_ARG
        assert _call(lib, name, p, xi=None, **kw) == _lib.FA_ERR_ARG
        assert _call(lib, name, p, out=p + 8, **kw) == _lib.FA_ERR_ARG
        assert _call(lib, name, p, tiles=1 << 31, **kw) == _lib.FA_ERR_ARG
        # nothing to fold: no launch, FA_OK
        assert _call(lib, name, p, L=0, **kw) == _lib.FA_OK
        assert _call(lib, name, p, tiles=0, **kw) == _lib.FA_OK
    if form:
        assert _call(lib, name, p, dtype=4) == _lib.FA_ERR_ARG
        assert _call(lib, name, p, dtype=-1) == _lib.FA_ERR_ARG
        assert _call(lib, name, p, dtype=0, cap=-1) == _lib.FA_ERR_ARG
        assert b"grid cap" in lib.fa_bench_last_error()
    else:
        with pytest.raises(_lib.InsufficientClientResults):
            _lib.check(_call(lib, name, p, N=0), name)
        # the same refusals as the one-layer row-table fold of the dtype
        one = {"fa_fedavg_f32_layers": lambda N: lib.fa_fedavg_f32_ptrs(p, N, 8, p, None, 1.0, p, None),
               "fa_fedavg_bf16_layers": lambda N: lib.fa_fedavg_bf16_ptrs(p, N, 8, p, None, 1.0, 1, p, None, None),
               "fa_fedavg_f16_layers": lambda N: lib.fa_fedavg_f16_ptrs(p, N, 8, p, None, 0x3C00, 1, p, None),
               "fa_fedavg_f64_layers": lambda N: lib.fa_fedavg_f64_ptrs(p, N, 8, p, None, 1.0, 1, p, None)}[name]
        for N in (0, -1):
            rc1 = one(N)
            msg1 = _lib.last_error()
            assert _call(lib, name, p, N=N) == rc1 != _lib.FA_OK
            if N == 0:
                assert _lib.last_error() == msg1
