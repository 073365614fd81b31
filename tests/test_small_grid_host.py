"""The bench library's CU-count override (fa_bench_set_cus) without a GPU,
where cu_count() falls back to 256: the override reaches the fp32 shape
policy, clearing it restores the real answer, the product library has no
setter; and the host side of tests/test_gpu_small_grid.py: tile widths read
off the form tables, the widths and band counts it runs at, the span condition
of its expectations and the coverage of its step tables."""
import ctypes
import os

import numpy as np
import pytest

import edge_values as E
import small_grid as SG
from fedlesscan_amd import _lib
from oracle import oracle_lib as OL  # checker

NS_PICK = [1, 10, 23, 24, 47, 48, 64, 100, 112, 255, 256, 1024]
PS_PICK = [4099, 32768, 40000, 81920, 262144, 300_003, 582_000, 800_000, 1_000_000, 2_100_003, 4_194_304, 25_000_000]


@pytest.fixture()
def B():
    b = _lib.load_bench()
    assert b.fa_bench_set_cus(0) == 0
    yield b
    assert b.fa_bench_set_cus(0) == 0, "a test left the override set"


def _picks(B, cus):
    return [B.fa_f32_pick_name(N, P, cus) for N in NS_PICK for P in PS_PICK]


def test_override_reaches_the_policy_and_clears(B):
    real = _picks(B, 0)
    assert real == _picks(B, 256) and all(real)  # no GPU: 256 CUs
    prev = 0
    for K in (2, 3, 64, 304):
        assert B.fa_bench_set_cus(K) == prev  # the setter returns the previous value
        prev = K
        got = _picks(B, 0)
        assert got == _picks(B, K), K
        assert got != real, (K, "the grid of shapes does not tell this CU count from 256")
    assert B.fa_bench_set_cus(-5) == 304  # negative: the real count
    assert B.fa_bench_set_cus(0) == 0
    assert _picks(B, 0) == real


def test_product_library_has_no_setter():
    L = _lib.load()
    for name in ("fa_bench_set_cus", "fa_set_cus", "fa_bench_fold_f32"):
        assert not hasattr(L, name), name
    assert "fa_bench_set_cus" not in _lib.header_functions()
    assert "fa_bench_set_cus" in _lib.header_functions(_lib.BENCH_HEADER)
    # the product's policy never moves with the bench library's override
    B = _lib.load_bench()
    before = [L.fa_fold_form(0, N, P, P, 0, None) for N in (10, 300) for P in (582_000, 2_100_003)]
    try:
        B.fa_bench_set_cus(2)
        assert [L.fa_fold_form(0, N, P, P, 0, None) for N in (10, 300) for P in (582_000, 2_100_003)] == before
    finally:
        B.fa_bench_set_cus(0)


def test_twins_are_declared_and_check_as_the_product(B):
    for name in ("fa_bench_set_cus", "fa_bench_fold_f32", "fa_bench_fold_f16", "fa_bench_fold_f64",
                 "fa_bench_fedavg_f64_ptrs"):
        assert name in _lib._BENCH_PROTOS and name in _lib.header_functions(_lib.BENCH_HEADER) and hasattr(B, name)
    L = _lib.load()
    x = ctypes.create_string_buffer(64)
    p = ctypes.addressof(x)
    for fb, fl, d in ((B.fa_bench_fold_f32, L.fa_fold_f32, 1.0), (B.fa_bench_fold_f16, L.fa_fold_f16, 0x3C00),
                      (B.fa_bench_fold_f64, L.fa_fold_f64, 1.0)):
        for args in ((p, 0, 4, 4, p, None, None, d, 1, p, None),   # N == 0 without an accumulator
                     (p, 2, 4, 3, p, None, None, d, 1, p, None),   # pitch below P
                     (None, 2, 4, 4, p, None, None, d, 1, p, None),
                     (p, 2, -1, 4, p, None, None, d, 1, p, None),
                     (p, 2, 0, 4, p, None, None, d, 1, p, None)):  # P == 0: nothing to do
            assert fb(*args) == fl(*args), args
    for args in ((p, 0, 4, p, None, 1.0, 1, p, None), (None, 2, 4, p, None, 1.0, 1, p, None),
                 (p, 2, 0, p, None, 1.0, 0, p, None)):
        assert B.fa_bench_fedavg_f64_ptrs(*args) == L.fa_fedavg_f64_ptrs(*args), args


# ---------------------------------------------------------------------------
# the shapes of tests/test_gpu_small_grid.py
# ---------------------------------------------------------------------------
def test_tiles_read_off_the_form_tables(B):
    assert SG.largest_tiles(B) == {"f32": 8192, "bf16": 16384, "f16": 16384, "f64": 2048}
    assert SG.tile_columns("gs1b512_u8c2nt_nts", 4) == 4096 and SG.tile_columns("gsw64_u24c2", 4) == 512
    assert SG.tile_columns("tile_16k_ps", 4) == 4096 and SG.tile_columns("lds2_w4r32t40", 4) == 160


def test_every_form_is_classified(B):
    """A form is a policy entry, the occupancy-sized balanced variant, one whose
    grid does not follow the CU count, or one whose geometry is restated."""
    n = SG.form_names(B)
    seen_bands = 0
    for fam, names in n.items():
        if fam.startswith("step"):
            assert all(x in SG.STEP_SPECS for x in names), (fam, names)
            continue
        for x in names:
            kinds = [x in ("auto", "bf16auto"), x == "bal_u4c4nt", SG.cu_independent(x),
                     SG.tiles_per_block(x, 1 << 20, 2, 4) is not None]
            assert sum(kinds) == 1, (fam, x, kinds)
            seen_bands += SG.band_form(x) is not None
    assert seen_bands >= 4 + 2 + 8 + 5 + 5  # fp32 variants and forms, bf16 variants and forms, f16 forms


@pytest.mark.parametrize("K", SG.KS)
def test_widths_give_three_tiles_per_block_and_three_bands(B, K):
    n, G = SG.form_names(B), 2 * K
    m = SG.pick_m(B, K)
    assert m % G == 0 and m >= 3 * G
    fams = {"f32": n["f32_variants"] + n["f32_forms"] + n["ptrs_forms"],
            "bf16": n["bf16_variants"] + n["bf16_forms"] + n["rows16_forms"], "f16": n["f16_forms"]}
    for kind, names in fams.items():
        T, u = SG.largest_tiles(B)[kind], SG.UNIT[kind]
        ws = SG.widths(B, kind, K)
        assert ws[0] % T == 0 and ws[1] % T == 2 * u - 1 and ws[2] % T == SG.KBLOCK * u + u // 2
        assert 100_000 <= ws[0] and ws[2] <= 500_000
        for P in ws:
            assert P // T >= 3 * G
            for x in names:
                tb = SG.tiles_per_block(x, P, K, u)
                if tb is None:
                    continue
                bf = SG.band_form(x)
                if bf is None:
                    assert tb[0] >= 3, (x, P, tb)
                    continue
                # a band launch is `passes` tiles per block by construction: a 2-pass form holds two
                assert tb[0] >= min(3, bf[1]) and tb[1] >= 2, (x, P, tb)
                if bf[1] == 4 or (kind == "f32" and bf[1] == 6):
                    assert tb[1] >= 3, (x, P, tb)
    # float64: the pair folds' balanced grid is at most one block per CU
    P64 = SG.widths(B, "f64", K)
    for P in P64:
        assert P // 2048 >= 3 * G and SG.ceil_div(SG.n_tiles(P, 4, 2), K) >= 3


def test_the_case_list(B):
    cs = SG.cases()
    assert {(N, w) for K, N, w in cs if K == 2} == {(N, w) for N in SG.NS for w in range(3)
                                                    if N in SG.NS_ALL_WIDTHS or w == 1}
    assert [c for c in cs if c[0] == 3] == [(3, 10, 1)]
    # the rows after the first, in groups of U rows in flight: for every U some count leaves no full group,
    # some a whole number of groups, some (U <= 8) groups and leftover rows; exactly one group at U = 8 and 16,
    # exactly two at U = 4, 8 and 16
    rest = [N - 1 for N in SG.NS]
    for U in (2, 4, 8, 16):
        assert any(r < U for r in rest) and any(r >= U and r % U == 0 for r in rest), U
        assert U == 16 or any(r > U and r % U for r in rest), U
        assert (U in rest) == (U >= 8) and (2 * U in rest) == (U >= 4), U


@pytest.mark.parametrize("kind", ["f32", "bf16", "f64", "f16"])
def test_every_expectation_meets_the_span_condition(B, kind):
    """Checked here for every (K, N, width) the GPU test runs, so its own check
    before the launches cannot be the first to see a seed that misses."""
    T = SG.largest_tiles(B)[kind]
    for K, N, w in SG.cases():
        P = SG.widths(B, kind, K)[w]
        X = SG.matrix(kind, N, P)
        if kind == "f16":
            for fid, ws, sc in SG.f16_factor_sets(N):
                exp = SG.numpy_fold_f16(X, ws, sc)
                assert SG.span_condition(exp, T, not any(ws)), (kind, K, N, P, fid)
            continue
        for fid, a, s, d in SG.factor_sets(N, np.float64 if kind == "f64" else np.float32):
            if kind == "f32":
                exp = OL.fedavg_f32(X, a, d, s=s)
            elif kind == "f64":
                exp = OL.fedavg_f64(X, a, d, s=s)
            else:
                exp, eb = OL.fedavg_bf16(X, a, d, s=s)
                assert E.bf16_matches_independent(eb, exp)
            assert SG.span_condition(exp, T, not a.any()), (kind, K, N, P, fid)


@pytest.mark.parametrize("K", SG.KS)
def test_step_tables_cover_every_column_once(B, K):
    n = SG.form_names(B)
    for fam in ("step_forms", "step_forms_f16", "step_forms_f64"):
        for name in n[fam]:
            kind = "bf16" if name.startswith("bf16") else name.split("_")[0]
            for P in SG.widths(B, kind, K):
                offs = SG.step_offsets(kind, P)
                assert all(o % 64 == 0 for o in offs[:-1]) and offs[-1] == P
                count, held = SG.step_coverage(name, offs, K)
                assert (count == 1).all(), (name, P, np.flatnonzero(count != 1)[:4])
                assert held >= 2, (name, P, held)  # a block holds several wide tiles of one round


def test_header_documents_the_override():
    with open(os.path.join(_lib.REPO, "include", "fedavg_hip_bench.h")) as f:
        text = f.read()
    assert "int fa_bench_set_cus(int cus);" in text and "previous value" in text
